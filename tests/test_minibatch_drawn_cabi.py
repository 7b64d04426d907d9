"""The two entry points of the drawn minibatches are exported, declared in include/ptg_env.h and refuse a null handle; no GPU needed."""
import os
import re

from rl_ptg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_exported_and_refuse_a_null_handle():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "ptg_env.h")).read()
    for name in ("ptg_minibatch_drawn", "ptg_minibatch_end_epoch"):
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"^int %s\(ptg_env\* env, uint64_t\* cursor_dev" % name, hdr, re.M)
    assert L.ptg_minibatch_drawn(None, None, 0, None, 1, 1, None, 0, 0, 0, 0, 0, None, 0, None, None, None, None) == _lib.E_INVALID
    assert L.ptg_minibatch_end_epoch(None, None, None) == _lib.E_INVALID
    assert L.ptg_abi_version() == 13                         # additive: nothing earlier changed
