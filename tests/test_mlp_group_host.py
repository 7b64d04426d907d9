"""ptg_mlp_group_forward / ptg_mlp_group_backward without a device: the exported symbols, the refusals the library makes on a NULL handle,
every Python-level refusal of HipEngine.mlp_group_forward / mlp_group_backward (TypeError across all networks before the ValueError of any,
the single op's words behind "net i:", nothing touched), the descriptor arrays an accepted call hands the library, DeviceMLPGroup /
TrainMLPGroup on CPU modules, and a group of one against the single op: the same descriptor bytes, the same refusals, the same backward plan.  The arithmetic has no test here: a grouped call is defined as the single calls, which tests/test_mlp_group.py
compares bit for bit on the device."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(fan_in, widths):
    from helpers import mlp_layers
    return mlp_layers(fan_in, widths)


def _ws(eng, B, widths, keep=True):
    import torch
    return torch.zeros(eng.mlp_workspace(B, widths, keep), dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------- the ABI, without a device
def test_the_library_exports_both_symbols_and_the_abi_stays():
    from rl_ptg_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, n) and n in _lib.EXPORTS for n in ("ptg_mlp_group_forward", "ptg_mlp_group_backward"))
    assert L.ptg_abi_version() == 13
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    assert "#define PTG_MLP_GROUP_MAX 8" in hdr and _lib.MLP_GROUP_MAX == 8
    assert "int ptg_mlp_group_forward(ptg_env* env, const ptg_mlp* nets, int32_t n_nets, void* stream);" in hdr
    assert "int ptg_mlp_group_backward(ptg_env* env, const ptg_mlp_bwd* nets, int32_t n_nets, void* stream);" in hdr


def test_a_null_handle_a_null_array_and_a_count_out_of_range_without_a_device():
    """no handle exists without a device, so the array and the counts are given to a NULL handle here; with a handle they are refused one
    by one in tests/test_mlp_group.py"""
    from rl_ptg_amd import _lib
    L = _lib.lib()
    f, b = (_lib.PtgMlp * 9)(), (_lib.PtgMlpBwd * 9)()
    for n in (0, 1, 8, 9, -1):
        assert L.ptg_mlp_group_forward(None, f, n, None) == _lib.E_INVALID
        assert L.ptg_mlp_group_backward(None, b, n, None) == _lib.E_INVALID
    assert L.ptg_mlp_group_forward(None, None, 1, None) == _lib.E_INVALID and L.ptg_mlp_group_backward(None, None, 1, None) == _lib.E_INVALID


# ------------------------------------------------------------------------------------------------- the Python argument checks
def _good(eng, B=6, G=2):
    """the arguments of a good grouped forward and backward: 41 (40 + 1) -> 8 -> 8 -> 5 and then 7 -> 9 -> 9 -> 2 ..."""
    import torch
    fwd = dict(xs=[], x2s=[], weights=[], biases=[])
    bwd = dict(grad_outs=[], outs=[], workspaces=[])
    for i in range(G):
        f1, f2, widths = (40, 1, [8, 8, 5]) if i == 0 else (6 + i, 0, [9, 9, 1 + i])
        w, b = _net(f1 + f2, widths)
        fwd["xs"].append(torch.zeros(B, f1))
        fwd["x2s"].append(torch.zeros(B, f2) if f2 else None)
        fwd["weights"].append(w)
        fwd["biases"].append(b)
        bwd["grad_outs"].append(torch.zeros(B, widths[-1]))
        bwd["outs"].append(torch.zeros(B, widths[-1]))
        bwd["workspaces"].append(_ws(eng, B, widths))
    return fwd, bwd


def test_python_refusals_touch_nothing():
    import torch
    from helpers import host_engine
    eng = host_engine(4)
    B = 6
    fwd, bwd = _good(eng, B, 3)
    t, v = TypeError, ValueError
    sub = lambda xs, i, e: xs[:i] + [e] + xs[i + 1:]
    F = lambda **kw: {**fwd, **kw}
    x0 = fwd["xs"][0]
    cases = [
        # a TypeError in network 1 is reported before a ValueError in network 0
        (t, "net 1:", F(xs=[torch.zeros(B, 2, 3), fwd["xs"][1].double(), fwd["xs"][2]])),
        (t, "net 2:", F(xs=[torch.zeros(B, 39), fwd["xs"][1], fwd["xs"][2]], biases=sub(fwd["biases"], 2, sub(fwd["biases"][2], 1, None)))),
        (v, "net 0:", F(xs=sub(fwd["xs"], 0, torch.zeros(B, 39)))),
        # the containers
        (t, "weights and biases", F(weights=fwd["weights"][0][0])), (t, "net 1:", F(weights=sub(fwd["weights"], 1, fwd["weights"][1][0]))),
        (t, "xs must be", F(xs=None)), (t, "outs must be", F(outs=torch.zeros(B, 5))), (t, "x2s must be", F(x2s=x0)),
        # list lengths that disagree, more than 8 networks, an empty group
        (v, "xs must have one entry per network, 3, got 2", F(xs=fwd["xs"][:2])), (v, "biases must have one entry per network", F(biases=fwd["biases"][:2])),
        (v, "x2s must have", F(x2s=[None] * 4)), (v, "outs must have", F(outs=[None])), (v, "workspaces must have", F(workspaces=[])),
        (v, "1 to 8 networks, got 9", dict(xs=x0, x2s=[fwd["x2s"][0]] * 9, weights=[fwd["weights"][0]] * 9, biases=[fwd["biases"][0]] * 9)),
        (v, "1 to 8 networks, got 0", dict(xs=[], weights=[], biases=[])),
        # unequal batch, unequal depth
        (v, "nets 0 and 2 disagree in the batch: 6 and 7 rows", F(xs=sub(fwd["xs"], 2, torch.zeros(B + 1, 8)))),
        (v, "nets 0 and 1 disagree in depth: 3 and 2 layers", F(weights=sub(fwd["weights"], 1, _net(7, [9, 2])[0]), biases=sub(fwd["biases"], 1, _net(7, [9, 2])[1]))),
        # activations belong to the whole group
        (v, "hidden_activation", F(hidden_activation="gelu")), (v, "out_activation", F(out_activation="sigmoid")),
        # outputs and workspaces
        (v, "net 1: out must be", F(outs=[None, torch.zeros(B, 3), None])), (v, "net 2: workspace has", F(workspaces=[None, None, torch.zeros(8, dtype=torch.uint8)])),
    ]
    shared_out = torch.zeros(B, 5)
    same = dict(xs=x0, x2s=[fwd["x2s"][0]] * 2, weights=[fwd["weights"][0]] * 2, biases=[fwd["biases"][0]] * 2)
    w = _ws(eng, B, [8, 8, 5], False)
    cases += [(v, "start at the same address", {**same, "outs": [shared_out, shared_out]}), (v, "start at the same address", {**same, "workspaces": [w, w]})]
    for k, (exc, text, kw) in enumerate(cases):
        with pytest.raises(exc, match=text) as e:
            eng.mlp_group_forward(**kw)
        assert type(e.value) is exc and str(e.value).startswith("mlp_group_forward: "), (k, str(e.value))
        assert eng._L is None, k
    # the backward: its own arguments
    G3 = lambda **kw: {**fwd, **bwd, **kw}
    gw = [[torch.zeros_like(w) for w in ws] for ws in fwd["weights"]]
    gb = [[torch.zeros_like(b) for b in bs] for bs in fwd["biases"]]
    one = torch.zeros(eng.mlp_backward_workspace(B, [9, 9, 3]), dtype=torch.uint8)
    gx = torch.zeros(B, 8)
    cases = [
        (t, "net 2:", G3(grad_outs=sub(bwd["grad_outs"], 2, bwd["grad_outs"][2].double()), xs=sub(fwd["xs"], 0, torch.zeros(B, 39)))),
        (t, "net 1: grad_weights and grad_biases go together", G3(grad_weights=[gw[0], gw[1], None], grad_biases=[gb[0], None, None])),
        (t, "grad_outs must be", G3(grad_outs=bwd["grad_outs"][0])), (t, "workspaces must be", G3(workspaces=None)),
        (v, "grad_outs must have", G3(grad_outs=bwd["grad_outs"][:2])), (v, "grad_xs must have", G3(grad_xs=[None])),
        (v, "net 1: grad_x2 without x2", G3(grad_x2s=[None, torch.zeros(B, 1), None])),
        (v, "net 2: grad_x must be", G3(grad_xs=[None, None, torch.zeros(B, 9)])),
        (v, "net 1: grad_weights\\[1\\] and grad_biases\\[1\\] go together", G3(grad_weights=[None, sub(gw[1], 1, None), None], grad_biases=[None, gb[1], None])),
        (v, "net 1: grad_weights\\[0\\] must be", G3(grad_weights=[None, sub(gw[1], 0, torch.zeros(9, 8)), None], grad_biases=[None, gb[1], None])),
        (v, "net 2: out must be", G3(outs=sub(bwd["outs"], 2, torch.zeros(B, 4)))),
        (v, "net 1: workspace has", G3(workspaces=sub(bwd["workspaces"], 1, torch.zeros(16, dtype=torch.uint8)))),
        (v, "net 2: backward_workspace has", G3(backward_workspaces=[None, None, one[:-1]])),
        (v, "nets 0 and 1 disagree in the batch", G3(xs=sub(fwd["xs"], 1, torch.zeros(B + 1, 7)), grad_outs=sub(bwd["grad_outs"], 1, torch.zeros(B + 1, 2)),
                                                      outs=sub(bwd["outs"], 1, torch.zeros(B + 1, 2)), workspaces=sub(bwd["workspaces"], 1, _ws(eng, B + 1, [9, 9, 2])))),
        # one tensor given twice among the outputs of different networks
        (v, "start at the same address", G3(backward_workspaces=[None, one, one])),
        (v, "start at the same address", G3(grad_xs=[None, None, gx], grad_weights=[None, gw[1], gw[2]], grad_biases=[None, sub(gb[1], 0, gb[2][0]), gb[2]])),
    ]
    twin = dict(grad_outs=[bwd["grad_outs"][0]] * 2, outs=[bwd["outs"][0], torch.zeros(B, 5)], workspaces=[bwd["workspaces"][0], _ws(eng, B, [8, 8, 5])], **same)
    cases += [(v, "start at the same address", {**twin, "grad_weights": [gw[0], gw[0]], "grad_biases": [gb[0], [torch.zeros_like(b) for b in gb[0]]]}),
              (v, "start at the same address", {**twin, "grad_xs": [torch.zeros(B, 40)] * 2})]
    for k, (exc, text, kw) in enumerate(cases):
        with pytest.raises(exc, match=text) as e:
            eng.mlp_group_backward(**kw)
        assert type(e.value) is exc and str(e.value).startswith("mlp_group_backward: "), (k, str(e.value))
        assert eng._L is None, k


def test_every_single_op_refusal_in_a_non_first_network_with_its_prefix():
    """helpers.faulty_mlp_nets, all 37: each faulty net as network 1 (and as network 2 of the backward) behind a good network 0: the single
    op's exception class and its words behind "net 1: ".  The four entries whose fault is an activation name concern the whole group, which
    reports them for network 0"""
    import torch
    from helpers import faulty_mlp_nets, host_engine
    eng = host_engine(4)
    B = 6
    nets = faulty_mlp_nets(B)
    assert len(nets) == 37
    good_w, good_b = _net(7, [9, 9, 2])
    good = dict(x=torch.zeros(B, 7), x2=None, weights=good_w, biases=good_b)
    rest = dict(grad_out=torch.zeros(B, 5), out=torch.zeros(B, 5), workspace=_ws(eng, B, [8, 8, 5]))
    good_rest = dict(grad_out=torch.zeros(B, 2), out=torch.zeros(B, 2), workspace=_ws(eng, B, [9, 9, 2]))
    n_act = 0
    for k, (exc, kw) in enumerate(nets):
        acts = {a: kw[a] for a in ("hidden_activation", "out_activation") if a in kw}
        with pytest.raises(exc) as single:
            eng.mlp_forward(**kw)
        text = str(single.value)
        assert text.startswith("mlp_forward: ")
        net1 = {**dict(x2=None), **{a: b for a, b in kw.items() if a not in acts}}
        group = dict(xs=[good["x"], net1["x"]], x2s=[None, net1["x2"]], weights=[good_w, net1["weights"]], biases=[good_b, net1["biases"]], **acts)
        with pytest.raises(exc) as fwd:
            eng.mlp_group_forward(**group)
        with pytest.raises(exc) as bwd:
            eng.mlp_group_backward(grad_outs=[good_rest["grad_out"], rest["grad_out"]], outs=[good_rest["out"], rest["out"]], workspaces=[good_rest["workspace"], rest["workspace"]], **group)
        assert type(fwd.value) is exc and type(bwd.value) is exc
        if acts and exc is ValueError:                       # an activation name: the group's, found at network 0
            n_act += 1
            assert str(fwd.value) == "mlp_group_forward: net 0: " + text[len("mlp_forward: "):], (k, str(fwd.value))
        else:
            assert str(fwd.value) == "mlp_group_forward: net 1: " + text[len("mlp_forward: "):], (k, text, str(fwd.value))
            assert str(bwd.value) == "mlp_group_backward: net 1: " + text[len("mlp_forward: "):], (k, text, str(bwd.value))
        assert eng._L is None, k
    assert n_act == 3


def test_accepted_calls_reach_the_library_once_with_every_field_of_every_network():
    """a shared x, a strided x2, a frozen layer in network 0 only, dx wanted for network 1 only"""
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B = 17
    wide = torch.zeros(B, 50)
    x, x2 = wide[:, :40], wide[:, 45:46]                     # x: shared by both networks; x2: network 0's second piece, row stride 50
    widths = [[233, 37, 5], [33, 17, 1]]
    nets = [_net(41, widths[0]), _net(40, widths[1])]
    weights, biases = [n[0] for n in nets], [n[1] for n in nets]
    outs = [torch.zeros(B, 8)[:, 1:6], torch.zeros(B, 1)]
    works = [_ws(eng, B, w) for w in widths]
    res = eng.mlp_group_forward(x, weights, biases, hidden_activation="tanh", out_activation="tanh", x2s=[x2, None], outs=outs, workspaces=works, keep_hidden=True)
    assert [c[0] for c in eng._L.calls] == ["ptg_mlp_group_forward"]
    _, descs, G, stream = eng._L.calls[0][1]
    assert G == 2 and stream is None and len(descs) == 2 and isinstance(descs[0], _lib.PtgMlp)
    for i, d in enumerate(descs):
        assert (d.batch, d.n_layers, d.flags, d.hidden_act, d.out_act) == (B, 3, _lib.MLP_KEEP_HIDDEN, _lib.MLP_TANH, _lib.MLP_TANH), i
        assert (d.x_dev, d.x_s_n) == (x.data_ptr(), 50) and (d.out_dev, d.out_s_n) == (outs[i].data_ptr(), (8, 1)[i]), i
        assert (d.ws_dev, d.ws_bytes) == (works[i].data_ptr(), works[i].numel()), i
        assert list(d.w_dev)[:4] == [w.data_ptr() for w in weights[i]] + [None] and list(d.b_dev)[:3] == [b.data_ptr() for b in biases[i]], i
        assert list(d.width)[:4] == widths[i] + [0] and list(d.w_s_n)[:3] == [(41, 40)[i]] + widths[i][:2], i
    assert (descs[0].f1, descs[0].f2, descs[0].x2_dev, descs[0].x2_s_n) == (40, 1, x2.data_ptr(), 50)
    assert (descs[1].f1, descs[1].f2, descs[1].x2_dev, descs[1].x2_s_n) == (40, 0, None, 0)
    assert len(res) == 2 and all(r.out.data_ptr() == o.data_ptr() for r, o in zip(res, outs))
    assert [h.shape for h in res[0].hidden] == [(B, 233), (B, 37)] and [h.stride(0) for h in res[0].hidden] == [236, 40]
    assert res[1].hidden[1].data_ptr() == works[1].data_ptr() + 4 * B * 36
    # without keep_hidden and without buffers: allocated per network, flags 0
    eng._L.calls.clear()
    res = eng.mlp_group_forward([x, x], weights, biases, x2s=[x2, None])
    d = eng._L.calls[0][1][1]
    assert [e.flags for e in d] == [0, 0] and [e.ws_bytes for e in d] == [2 * B * 236 * 4, 2 * B * 36 * 4] and res[0].hidden is None and res[1].out.shape == (B, 1)
    assert d[0].out_dev != d[1].out_dev and d[0].ws_dev != d[1].ws_dev
    # the backward
    eng._L.calls.clear()
    gouts = [torch.zeros(B, 8)[:, 2:7], torch.zeros(B, 1)]
    gws, gbs = [[torch.zeros_like(w) for w in ws] for ws in weights], [[torch.zeros_like(b) for b in bs] for bs in biases]
    gpad = torch.zeros(233, 48)
    gws[0][0] = gpad[:, :41]                                 # a weight gradient with a row stride above its fan-in
    gws[0][1], gbs[0][1] = None, None                        # frozen in network 0 only
    gx1 = torch.zeros(B, 44)[:, :40]
    bws1 = torch.zeros(eng.mlp_backward_workspace(B, widths[1]) + 4, dtype=torch.uint8)
    ret = eng.mlp_group_backward(gouts, x, weights, biases, outs, works, hidden_activation="tanh", out_activation="tanh", x2s=[x2, None], grad_weights=gws, grad_biases=gbs,
                                 grad_xs=[None, gx1], backward_workspaces=[None, bws1], accumulate=True)
    assert [c[0] for c in eng._L.calls] == ["ptg_mlp_group_backward"]
    _, descs, G, stream = eng._L.calls[0][1]
    assert G == 2 and len(descs) == 2 and isinstance(descs[0], _lib.PtgMlpBwd) and len(ret) == 2 and ret[1] is bws1
    for i, d in enumerate(descs):
        fw = d.fwd
        assert (fw.batch, fw.n_layers, fw.flags, fw.hidden_act, fw.out_act, fw.f1, fw.f2) == (B, 3, _lib.MLP_KEEP_HIDDEN, _lib.MLP_TANH, _lib.MLP_TANH, 40, 1 - i), i
        assert (fw.x_dev, fw.x_s_n, fw.out_dev, fw.ws_dev, fw.ws_bytes) == (x.data_ptr(), 50, outs[i].data_ptr(), works[i].data_ptr(), works[i].numel()), i
        assert list(fw.w_dev)[:3] == [w.data_ptr() for w in weights[i]] and list(fw.width)[:3] == widths[i], i
        assert (d.gout_dev, d.gout_s_n, d.flags) == (gouts[i].data_ptr(), (8, 1)[i], _lib.MLP_ACCUMULATE), i
        assert (d.bws_dev, d.bws_bytes) == (ret[i].data_ptr(), ret[i].numel()), i
        assert list(d.dw_dev)[:4] == [None if g is None else g.data_ptr() for g in gws[i]] + [None], i
        assert list(d.db_dev)[:3] == [None if g is None else g.data_ptr() for g in gbs[i]], i
    assert list(descs[0].dw_s_n)[:3] == [48, 0, 37] and list(descs[1].dw_s_n)[:3] == [40, 33, 17]
    assert (descs[0].dx_dev, descs[0].dx2_dev, descs[1].dx_dev, descs[1].dx_s_n, descs[1].dx2_dev) == (None, None, gx1.data_ptr(), 44, None)
    assert descs[0].fwd.x2_dev == x2.data_ptr() and descs[1].fwd.x2_dev is None and ret[0].numel() == 2 * B * 236 * 4


# ------------------------------------------------------------------------------------------------- the classes
def _modules():
    from torch import nn
    pi = [nn.Sequential(nn.Linear(40, 16), nn.Tanh(), nn.Linear(16, 16), nn.Tanh()), nn.Linear(16, 5)]
    vf = nn.Sequential(nn.Linear(40, 12), nn.Tanh(), nn.Linear(12, 12), nn.Tanh(), nn.Linear(12, 1))
    return pi, vf


def test_the_group_classes_parse_refuse_and_order_their_parameters():
    import torch
    from torch import nn
    from helpers import host_engine, recording_engine
    from rl_ptg_amd import DeviceMLPGroup, TrainMLPGroup
    pi, vf = _modules()
    t, v = TypeError, ValueError
    relu = nn.Sequential(nn.Linear(40, 12), nn.ReLU(), nn.Linear(12, 12), nn.ReLU(), nn.Linear(12, 1))
    refused = [(t, "nets must be a list", vf), (v, "1 to 8 networks, got 0", []), (v, "1 to 8 networks, got 9", [vf] * 9), (t, "Sigmoid", [vf, nn.Sequential(nn.Linear(4, 4), nn.Sigmoid())]),
               (v, "nets 0 and 1 disagree in depth: 3 and 2", [vf, nn.Sequential(nn.Linear(40, 4), nn.Tanh(), nn.Linear(4, 1))]),
               (v, "nets 0 and 2 disagree in the hidden activation: tanh and relu", [pi, vf, relu]),
               (v, "nets 0 and 1 disagree in the output activation: None and tanh", [vf, [vf, nn.Tanh()]]), (v, "no bias", [vf, nn.Linear(4, 4, bias=False)])]
    eng = host_engine(4)
    for cls in (DeviceMLPGroup, TrainMLPGroup):
        for k, (exc, text, m) in enumerate(refused):
            with pytest.raises(exc, match=text):
                cls(eng, m, batch=6)
            assert eng._L is None, k
        with pytest.raises(ValueError):
            cls(eng, [pi, vf], batch=0)
    one_layer = DeviceMLPGroup(recording_engine(4), [nn.Linear(4, 3), [nn.Linear(5, 2)]], batch=2)      # depth 1: no hidden activation to disagree in
    assert len(one_layer.nets) == 2
    eng = recording_engine(4)
    grp = DeviceMLPGroup(eng, [pi, vf], batch=8)
    x = torch.zeros(6, 40)
    a, b = grp(x)
    assert (a.shape, b.shape) == ((6, 5), (6, 1)) and a.data_ptr() == grp.nets[0].out.data_ptr() and b.data_ptr() == grp.nets[1].out.data_ptr()
    assert [c[0] for c in eng._L.calls] == ["ptg_mlp_group_forward"]
    d = eng._L.calls[0][1][1]
    assert list(d[0].w_dev)[:3] == [pi[0][0].weight.data_ptr(), pi[0][2].weight.data_ptr(), pi[1].weight.data_ptr()] and d[1].w_dev[0] == vf[0].weight.data_ptr()      # by reference
    assert d[0].flags == 0 and d[0].hidden_act == 1 and d[0].x_dev == d[1].x_dev == x.data_ptr()
    grp([x, torch.zeros(6, 40)])
    d = eng._L.calls[1][1][1]
    assert d[0].x_dev != d[1].x_dev
    with pytest.raises(ValueError):
        grp(torch.zeros(9, 40))
    with pytest.raises(ValueError):
        grp([x])
    # TrainMLPGroup
    eng = recording_engine(4)
    grp = TrainMLPGroup(eng, [pi, vf], batch=8)
    ps = grp.parameters()
    assert len(ps) == 12 and ps[0] is pi[0][0].weight and ps[5] is pi[1].bias and ps[6] is vf[0].weight and ps[11] is vf[4].bias
    assert eng._L.calls == []
    x = torch.zeros(6, 40, requires_grad=True)
    a, b = grp(x)
    assert a.grad_fn is not None and b.grad_fn is not None and grp.calls == 1 and eng._L.calls[0][1][1][0].flags == 1
    torch.autograd.backward([a, b], [torch.ones_like(a), torch.ones_like(b)])
    assert [c[0] for c in eng._L.calls] == ["ptg_mlp_group_forward", "ptg_mlp_group_backward"]
    _, d, G, _ = eng._L.calls[1][1]
    assert G == 2 and [e.dx_dev for e in d] == [n.grad_input.data_ptr() for n in grp.nets] and d[0].dx_dev != d[1].dx_dev
    assert list(d[1].dw_dev)[:3] == [g.data_ptr() for g in grp.nets[1].grad_weights]
    assert vf[0].weight.grad is not None and vf[0].weight.grad.data_ptr() != grp.nets[1].grad_weights[0].data_ptr() and x.grad.shape == (6, 40)
    # an unused output: its network is left out of the call and keeps .grad None; a frozen network launches no dw work; an input without
    # requires_grad gets no first-layer dx
    for p in ps:
        p.grad = None
    eng._L.calls.clear()
    a, b = grp(x)
    b.sum().backward()
    _, d, G, _ = eng._L.calls[1][1]
    assert G == 1 and d[0].fwd.out_dev == grp.nets[1].out.data_ptr() and all(p.grad is None for p in ps[:6]) and all(p.grad is not None for p in ps[6:])
    for p in ps[:6]:
        p.requires_grad_(False)
    eng._L.calls.clear()
    a, b = grp([x.detach(), x])
    torch.autograd.backward([a.sum(), b.sum()])
    _, d, G, _ = eng._L.calls[1][1]
    assert G == 2 and list(d[0].dw_dev) == [None] * 10 and d[0].dx_dev is None and d[1].dx_dev == grp.nets[1].grad_input.data_ptr() and d[1].dw_dev[0] is not None
    # the stale forward
    y = grp(x)
    grp(x)
    with pytest.raises(RuntimeError, match="latest forward"):
        y[1].sum().backward()


# ------------------------------------------------------------------------------------------------- a group of one is the single call
def test_a_group_of_one_hands_the_library_the_single_ops_descriptor_byte_for_byte():
    """B = 17, 41 (40 + a strided one-column x2) -> 233 -> 37 -> 5, tanh / tanh, a strided out, a weight gradient with row stride 48, layer 1
    frozen, grad_x only, accumulate: the ptg_mlp of mlp_forward and element 0 of mlp_group_forward's array for the same tensors are the
    same bytes, and so are the ptg_mlp_bwd of mlp_backward and of mlp_group_backward"""
    import torch
    from helpers import recording_engine
    from rl_ptg_amd import _lib
    eng = recording_engine(4)
    B, widths = 17, [233, 37, 5]
    wide = torch.zeros(B, 50)
    x, x2 = wide[:, :40], wide[:, 45:46]
    w, b = _net(41, widths)
    out, work = torch.zeros(B, 8)[:, 1:6], _ws(eng, B, widths)
    acts = dict(hidden_activation="tanh", out_activation="tanh")
    eng.mlp_forward(x, w, b, x2=x2, out=out, workspace=work, keep_hidden=True, **acts)
    eng.mlp_group_forward([x], [w], [b], x2s=[x2], outs=[out], workspaces=[work], keep_hidden=True, **acts)
    gout = torch.zeros(B, 8)[:, 2:7]
    gw, gb = [torch.zeros(233, 48)[:, :41], None, torch.zeros(5, 37)], [torch.zeros(233), None, torch.zeros(5)]
    gx, bws = torch.zeros(B, 44)[:, :40], torch.zeros(eng.mlp_backward_workspace(B, widths), dtype=torch.uint8)
    eng.mlp_backward(gout, x, w, b, out, work, x2=x2, grad_weights=gw, grad_biases=gb, grad_x=gx, backward_workspace=bws, accumulate=True, **acts)
    eng.mlp_group_backward([gout], [x], [w], [b], [out], [work], x2s=[x2], grad_weights=[gw], grad_biases=[gb], grad_xs=[gx], backward_workspaces=[bws],
                           accumulate=True, **acts)
    calls = eng._L.calls
    assert [c[0] for c in calls] == ["ptg_mlp_forward", "ptg_mlp_group_forward", "ptg_mlp_backward", "ptg_mlp_group_backward"]
    for single, group, kind in ((calls[0], calls[1], _lib.PtgMlp), (calls[2], calls[3], _lib.PtgMlpBwd)):
        one, (arr, G) = single[1][1]._obj, group[1][1:3]
        assert G == 1 and len(arr) == 1 and isinstance(one, kind) and isinstance(arr[0], kind)
        assert bytes(one) == bytes(arr[0]) and len(bytes(one)) == C.sizeof(kind)
    d = calls[3][1][1][0]                                    # and the bytes are not empty ones
    assert (d.fwd.x2_dev, d.fwd.x2_s_n, d.fwd.out_s_n, d.dw_s_n[0], d.dw_dev[1], d.dx_s_n, d.dx2_dev, d.flags) == (x2.data_ptr(), 50, 8, 48, None, 44, None, _lib.MLP_ACCUMULATE)


def test_every_single_op_refusal_in_a_group_of_one_with_its_prefix():
    """helpers.faulty_mlp_nets, all 37, as network 0 of a group of one: the single op's exception class and its words behind "net 0: ", the
    forward's against mlp_forward's and the backward's against mlp_backward's"""
    import torch
    from helpers import faulty_mlp_nets, host_engine
    eng = host_engine(4)
    B = 6
    nets = faulty_mlp_nets(B)
    assert len(nets) == 37
    rest = dict(grad_out=torch.zeros(B, 5), out=torch.zeros(B, 5), workspace=_ws(eng, B, [8, 8, 5]))
    for k, (exc, kw) in enumerate(nets):
        acts = {a: kw[a] for a in ("hidden_activation", "out_activation") if a in kw}
        group = dict(xs=[kw["x"]], x2s=[kw.get("x2")], weights=[kw["weights"]], biases=[kw["biases"]], **acts)
        with pytest.raises(exc) as single_f:
            eng.mlp_forward(**kw)
        with pytest.raises(exc) as single_b:
            eng.mlp_backward(**kw, **rest)
        with pytest.raises(exc) as fwd:
            eng.mlp_group_forward(**group)
        with pytest.raises(exc) as bwd:
            eng.mlp_group_backward(grad_outs=[rest["grad_out"]], outs=[rest["out"]], workspaces=[rest["workspace"]], **group)
        assert type(single_f.value) is exc and type(single_b.value) is exc and type(fwd.value) is exc and type(bwd.value) is exc, k
        assert str(single_f.value).startswith("mlp_forward: ") and str(single_b.value).startswith("mlp_backward: "), k
        assert str(fwd.value) == "mlp_group_forward: net 0: " + str(single_f.value)[len("mlp_forward: "):], (k, str(fwd.value))
        assert str(bwd.value) == "mlp_group_backward: net 0: " + str(single_b.value)[len("mlp_backward: "):], (k, str(bwd.value))
        assert eng._L is None, k


def _fields(d, names):
    """every field of a ctypes descriptor, nested structures and arrays included; a device pointer found in `names` as its name"""
    out = {}
    for name, _ in d._fields_:
        v = getattr(d, name)
        out[name] = _fields(v, names) if hasattr(v, "_fields_") else [names.get(e, e) for e in v] if hasattr(v, "__len__") else names.get(v, v)
    return out


@pytest.mark.parametrize("pattern", ["all parameters", "the last layer only", "the input only"])
def test_a_train_mlp_group_of_one_hands_the_library_what_train_mlp_does(pattern):
    """one module, 41 (40 + 1) -> 16 -> 12 -> 3, under a TrainMLP and under a TrainMLPGroup of one: the ptg_mlp_bwd of the two backward calls
    agree in every field, each object's own buffers (out, workspaces, gradient buffers) and autograd's grad_out taken by name"""
    import torch
    from torch import nn
    from helpers import recording_engine
    torch.manual_seed(0)
    module = nn.Sequential(nn.Linear(41, 16), nn.Tanh(), nn.Linear(16, 12), nn.Tanh(), nn.Linear(12, 3))
    params = list(module.parameters())
    for k, p in enumerate(params):
        p.requires_grad_(pattern == "all parameters" or (pattern == "the last layer only" and k >= 4))
    from rl_ptg_amd import TrainMLP, TrainMLPGroup
    B = 6
    x, x2 = torch.zeros(B, 40, requires_grad=pattern == "the input only"), torch.zeros(B, 1, requires_grad=pattern == "the input only")
    seen = []
    for grouped in (False, True):
        eng = recording_engine(4)
        obj = TrainMLPGroup(eng, [module], batch=8) if grouped else TrainMLP(eng, module, batch=8)
        net = obj.nets[0] if grouped else obj
        out = obj(x, x2=x2)[0] if grouped else obj(x, x2=x2)
        out.sum().backward()                                 # an expanded grad_out: both make it contiguous
        name, args = eng._L.calls[-1]
        assert name == ("ptg_mlp_group_backward" if grouped else "ptg_mlp_backward") and len(eng._L.calls) == 2
        d = args[1][0] if grouped else args[1]._obj
        assert not grouped or args[2] == 1
        names = {net.out.data_ptr(): "out", net.workspace.data_ptr(): "ws", net.backward_workspace.data_ptr(): "bws", net.grad_input.data_ptr(): "gx",
                 net.grad_input.data_ptr() + 4 * 40: "gx2", d.gout_dev: "gout"}
        names.update({t.data_ptr(): f"gw{l}" for l, t in enumerate(net.grad_weights)})
        names.update({t.data_ptr(): f"gb{l}" for l, t in enumerate(net.grad_biases)})
        seen.append(_fields(d, names))
        for p in params:
            p.grad = None
        x.grad = x2.grad = None
    single, group = seen
    assert single == group
    want = {"all parameters": ["gw0", "gw1", "gw2"], "the last layer only": [None, None, "gw2"], "the input only": [None, None, None]}[pattern]
    assert single["dw_dev"][:3] == want and single["db_dev"][:3] == [None if g is None else g.replace("w", "b") for g in want]
    assert (single["dx_dev"], single["dx2_dev"]) == (("gx", "gx2") if pattern == "the input only" else (None, None))
    assert single["gout_dev"] == "gout" and single["gout_s_n"] == 3 and single["fwd"]["w_dev"][:3] == [m.weight.data_ptr() for m in module if isinstance(m, nn.Linear)]
    assert single["fwd"]["out_dev"] == "out" and single["fwd"]["ws_dev"] == "ws" and single["bws_dev"] == "bws"
