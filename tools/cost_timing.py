"""What the *_cost.py tools share: device time of one call from HIP events, its summary, and two variants taken in turns."""
import statistics

_events = []


def timed(fn):
    """(device time of fn() [us], fn's result).  The section is queued behind a ~100 us device-side delay, so the host has enqueued its
    work (argument checks, ctypes, the launch) before the first event is reached: the events bracket device work only, not host latency
    on an idle stream."""
    import torch
    if not _events:
        _events.extend((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
    e0, e1 = _events
    torch.cuda._sleep(200000)                             # ~100 us of device time: the host runs ahead of the first event
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def stats(v, width=9):
    """median [min - max] of the times v"""
    return f"{statistics.median(v):{width}.1f} [{min(v):{width - 2}.1f} - {max(v):{width - 2}.1f}]"


def alternate(fa, fb, warmup, reps):
    """the times of fa and of fb, taken in turns: `reps` recorded repetitions after `warmup` unrecorded ones"""
    ta, tb = [], []
    for rep in range(warmup + reps):
        a, b = timed(fa)[0], timed(fb)[0]
        if rep >= warmup:
            ta.append(a); tb.append(b)
    return ta, tb
