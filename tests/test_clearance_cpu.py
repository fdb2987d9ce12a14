"""CPU: the clearance report (dmpc_postcheck_clearance) at the boundary -- the symbol and its binding, the ABI revision, the refusals that need
no device -- and the scenes of tests/test_gpu_clearance.py, held to what their tests assume with the oracle's post-check."""
import ctypes

import numpy as np
import pytest

import multiagent_planning_amd as mp
from multiagent_planning_amd import _lib
from oracle import postcheck as PC
import clearance as cl


def test_symbol_is_exported_and_the_abi_revision_stays_8():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dmpc_postcheck_clearance") and "dmpc_postcheck_clearance" in _lib.ABI_SYMBOLS
    assert lib.dmpc_abi_version() == 8 == _lib.ABI_VERSION
    L = _lib.load()
    assert len(L.dmpc_postcheck_clearance.argtypes) == 20 and L.dmpc_postcheck_clearance.argtypes[16] is ctypes.c_double      # reach
    assert callable(mp.Dmpc.clearance)


def test_null_context_is_refused_by_name():
    L = _lib.load()
    rc = L.dmpc_postcheck_clearance(None, 1, 2, 2, 5, None, None, None, None, None, None, None, 0, 2.0, 1.0, 0.01, float("inf"), None, None, None)
    assert rc == -1 and L.dmpc_last_error(None).decode().startswith("dmpc_postcheck_clearance: ")


def test_binding_refuses_path_together_with_po_static():
    with pytest.raises(mp.DmpcError, match="path and po_static exclude each other"):
        mp.Dmpc.clearance(None, [5], np.zeros((2, 3)), KT_alloc=5, po_static=np.zeros((1, 3)), path=np.zeros((1, 2, 3)))   # (raised before the context is used)


@pytest.mark.parametrize("n_cmd", [256, 257, 300])
def test_box_scene_has_slots_inside_and_outside_three_rmin(n_cmd):
    """the dense box of the regime-boundary test, through the oracle's post-check: of either kind some slots lie inside reach = 3 rmin and
    some do not, some pairs come within 2 rmin and most do not"""
    kw = cl.box_kw()
    pk, vk, ak, pos = cl.box_scene(n_cmd)
    o = PC.postcheck(pk, vk, ak, pk[:, -1], kw["h"], kw["rmin"], kw["c"])
    p = o["p"]
    assert (p >= np.array(kw["pmin"]) - 1.0).all() and (p <= np.array(kw["pmax"]) + 1.0).all()
    d0, d1 = cl.nearest(p, np.repeat(pos[:, None], p.shape[1], axis=1), kw["c"])
    for d in (d0, d1):
        assert 3 <= (d < cl.REACH3).sum() <= n_cmd - 3, ((d < cl.REACH3).sum(), n_cmd)
        assert np.abs(d - cl.REACH3).min() > 1e-6                                     # nobody sits on the bound
    assert 0 < (d0 < 2 * kw["rmin"]).sum() < n_cmd / 2
    assert abs(d0.min() - o["min_dist"]) <= 1e-12


@pytest.mark.parametrize("n", [4, 257])
def test_line_scene_is_an_exact_tie(n):
    """x is exact, has neither velocity nor acceleration, and all agents share one y-history: every neighbour is exactly 1 m away"""
    pk, vk, ak = cl.line_scene(n)
    assert np.array_equal(pk[:, :, 0], np.repeat(np.arange(n, dtype=float)[:, None], pk.shape[1], axis=1))
    assert not vk[:, :, 0].any() and not ak[:, :, 0].any() and not pk[:, :, 2].any()
    assert (pk[:, :, 1] == pk[0, :, 1]).all() and (vk[:, 0, 1] != 0).all()
    assert np.array_equal(cl.line_partner(4), [1, 0, 1, 2])
