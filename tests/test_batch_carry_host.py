"""Host side of the carry across states (mmw_batch_carry / mmw_batch_carry_map; no GPU): the entries are declared and exported, the
CPU restatement the GPU tests are held to (tests/helpers/carry_oracle.py) is itself checked against tests/helpers/warm_oracle.py on
identical states, the index maps the library merges from sorted rows equal the helper's, which looks keys up in a dictionary, on
three pairs of states, and the refusals a device -1 batch can reach answer with their status and leave both batches as they were."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, state_from
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import carry_oracle  # noqa: E402
import warm_oracle  # noqa: E402

from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.graphs import _state_at, mobile_drop  # noqa: E402

IFIELDS = (_lib.I_L_INDPTR, _lib.I_L_INDICES, _lib.I_ST_INDPTR, _lib.I_ST_INDICES, _lib.I_GAIN_X, _lib.I_GAIN_Y, _lib.I_ASSO_X, _lib.I_ASSO_Y,
           _lib.I_DIAG_POS, _lib.I_ASSO_POS)
HFIELDS = (_lib.F_S_SUM, _lib.F_NORM_H, _lib.F_ST_DATA)


def test_carry_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_carry(mmw_batch* dst, mmw_batch* src, const int32_t* take);" in hdr
    assert "int mmw_batch_carry_map(mmw_batch* dst, mmw_batch* src, int32_t inst, int32_t* lmap, int64_t nl, int32_t* cmap, int64_t nc);" in hdr
    for name in ("mmw_batch_carry", "mmw_batch_carry_map"):
        assert name in _lib.EXPORTS
        getattr(_lib.lib(), name)


def test_carry_oracle_on_identical_states_is_the_warm_oracle():
    g = load_golden("run_dense60")
    state, Z, eta = state_from(g), int(g["Z"]), float(g["eta"])
    K = state[0].shape[0]
    n1, n2, Z2 = 3, 2, Z + 1
    rng = np.random.default_rng(5)
    sk1 = [orc.sketch_rows(rng.standard_normal((K, 2 * Z))) for _ in range(n1)]
    sk2 = [orc.sketch_rows(rng.standard_normal((K, 2 * Z2))) for _ in range(n2)]
    c = carry_oracle.run(Z, n1, state, Z2, n2, state, eta, lambda i, K_, D: sk1[i], lambda i, K_, D: sk2[i])
    w = warm_oracle.run(Z, n1, Z2, n2, state, eta, lambda i, K_, D: sk1[i], lambda i, K_, D: sk2[i])
    for key in ("lval", "xval", "Y", "e_accu", "e_this", "X_half", "xsum", "ysum"):
        assert np.array_equal(c[key], w[key]), key
    lmap, cmap = carry_oracle.maps(c["pattern"], w["pattern"])
    assert np.array_equal(lmap, np.arange(lmap.size)) and np.array_equal(cmap, np.arange(cmap.size))


def pairs_of(p):
    return set(zip(p.asso_x.tolist(), p.asso_y.tolist()))


def entries_of(p):
    return set(zip(p.row.tolist(), p.col.tolist()))


def test_pair_a_loses_and_gains_entries_pairs_and_an_ap():
    """mobile_drop(5, 75e-4, 3) before and after step_time(1e6, 3.0): what makes it a test of the maps."""
    d = mobile_drop(5, 75e-4, carry_oracle.PAIR_A_SEED)
    asso0 = _state_at(d.sta_locs, d.ap_locs)[1]
    old, new = carry_oracle.moved_pair(5, carry_oracle.PAIR_A_SEED)
    d.step_time(1e6, 3.0)
    asso1 = _state_at(d.sta_locs, d.ap_locs)[1]
    po, pn = orc.Pattern(4, old), orc.Pattern(4, new)
    assert po.K == pn.K == 75
    assert entries_of(po) - entries_of(pn) and entries_of(pn) - entries_of(po)
    assert pairs_of(po) - pairs_of(pn) and pairs_of(pn) - pairs_of(po)
    assert np.any(asso0 != asso1)


def the_pairs():
    return {"a": carry_oracle.moved_pair(5, carry_oracle.PAIR_A_SEED), "b": carry_oracle.pair_b(), "c_lose": carry_oracle.pair_c("lose"),
            "c_gain": carry_oracle.pair_c("gain")}


@pytest.mark.parametrize("name", ["a", "b", "c_lose", "c_gain"])
def test_carry_map_is_the_helpers_map(name):
    old, new = the_pairs()[name]
    src = _lib.BatchSolver([3], [old], 3, 0.05, device=-1)
    dst = _lib.BatchSolver([4], [new], 3, 0.05, device=-1)  # any slot counts
    lmap, cmap = dst.carry_map(src, 0)
    po, pn = orc.Pattern(3, old), orc.Pattern(4, new)
    rl, rc = carry_oracle.maps(po, pn)
    assert np.array_equal(lmap, rl) and np.array_equal(cmap, rc)
    K, Eo, En = pn.K, po.E_asso, pn.E_asso
    assert np.array_equal(cmap[:K], np.arange(K)) and np.array_equal(cmap[K + En:], K + Eo + np.arange(K))
    assert np.all(lmap[pn.diag_pos] == po.diag_pos)
    if name == "b":
        off = np.ones(pn.nnzL, dtype=bool)
        off[pn.diag_pos] = False
        assert off.sum() == 6 and np.all(lmap[off] == -1) and np.all(cmap[K:K + En] == -1) and En == 2
    if name == "c_lose":
        assert (Eo, En) == (1, 0) and np.array_equal(lmap, [0, 1, 2, 3])  # (the gain edge sits where the pair sat: L carries, F is gone)
    if name == "c_gain":
        assert (Eo, En) == (0, 1) and cmap[K] == -1
    # and back: the map of the old state onto the new one's batch
    bl, bc = src.carry_map(dst, 0)
    ql, qc = carry_oracle.maps(pn, po)
    assert np.array_equal(bl, ql) and np.array_equal(bc, qc)
    src.close()
    dst.close()


def host_view(b):
    return [dict(s) for s in b.sizes], [[b.read_i32(i, f) for f in IFIELDS] + [b.read(i, f) for f in HFIELDS] for i in range(b.B)]


def unchanged(b, view):
    b._load_sizes()
    sz, fl = host_view(b)
    assert sz == view[0]
    for got, ref in zip(fl, view[1]):
        for a, r in zip(got, ref):
            assert np.array_equal(a, r)


def refused(status, text, call):
    with pytest.raises(_lib.MMWError, match=text) as e:
        call()
    assert ("status %d:" % status) in str(e.value), str(e.value)


def test_refusals_on_host_only_batches_leave_them_unchanged():
    old, new = carry_oracle.moved_pair(5, carry_oracle.PAIR_A_SEED)
    small = carry_oracle.pair_b()[0]
    src = _lib.BatchSolver([3, 3], [old, small], 3, 0.05, device=-1)
    dst = _lib.BatchSolver([4, 4], [new, new], 3, 0.05, device=-1)
    vs, vd = host_view(src), host_view(dst)
    refused(-1, "cannot carry from itself", lambda: dst.carry_from(dst))
    refused(-3, "host-only", lambda: dst.carry_from(src))
    refused(-3, "host-only", lambda: dst.carry_from(src, take=[1, 0]))
    refused(-1, "instance 1: K = 75 here, K = 4 in the source", lambda: dst.carry_map(src, 1))
    refused(-1, "out of range", lambda: check_map(dst, src, 2, 1, 1))
    refused(-1, "wrong lengths", lambda: check_map(dst, src, 0, dst.sizes[0]["nnzL"] - 1, dst.sizes[0]["C"]))
    refused(-1, "wrong lengths", lambda: check_map(dst, src, 0, dst.sizes[0]["nnzL"], dst.sizes[0]["C"] + 1))
    with pytest.raises(_lib.MMWError, match="one flag per instance"):
        dst.carry_from(src, take=[1])
    unchanged(src, vs)
    unchanged(dst, vd)
    src.close()
    dst.close()


def check_map(dst, src, inst, nl, nc):
    lmap, cmap = np.full(max(nl, 1) + 1, 7, dtype=np.int32), np.full(max(nc, 1) + 1, 7, dtype=np.int32)
    try:
        _lib.check(_lib.lib().mmw_batch_carry_map(dst._h, src._h, int(inst), _lib._pi(lmap), int(nl), _lib._pi(cmap), int(nc)))
    finally:
        assert np.all(lmap == 7) and np.all(cmap == 7)  # a refused call writes nothing
