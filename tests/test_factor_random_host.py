"""Host side of the random embedding on the solver handle (mmw_factor_random, `Solver.factor_random`,
`rand_sdp_solver(draws=)`; no GPU): the declaration and the export, every refusal a device = -1 handle can reach with the value it
names, the routing of `rand_sdp_solver` where no device is involved, and the kernel's width rule past 512 columns held to
`philox_ref._draw`.
"""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, state_from

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import philox_ref as pr  # noqa: E402

from sig_sdp_mmw_amd import _lib  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.sdp_solver import rand_sdp_solver, spectral_sdp_solver  # noqa: E402

DECLARATION = "int mmw_factor_random(mmw_solver* s, int32_t cols, int32_t index_order, double* out, uint64_t seed);"
MAX_COLS = 2 ** 31 - 1 - 64


def header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "mmw_hip.h")).read())


def last_error():
    return _lib.lib().mmw_last_error().decode()


def test_entry_is_declared_documented_exported_and_bound():
    txt = header()
    assert DECLARATION in txt
    assert txt.index("int mmw_factor_spectral(") < txt.index("int mmw_factor_random(") < txt.index("int mmw_expm_apply(")  # next to its sibling
    comment = txt[:txt.index("int mmw_factor_random(")].rsplit("/*", 1)[1]
    for cite in ("sdp_solver.py:109-114", "mmw_batch_factor_random", "0x4d4d5753", "MMW_F_FACTOR_ROWNORM", "MMW_FACTOR_RANDOM_MAX_COLS"):
        assert cite in comment, cite
    assert "#define MMW_FACTOR_RANDOM_MAX_COLS %d" % MAX_COLS in txt
    L = _lib.lib()
    assert "mmw_factor_random" in _lib.EXPORTS and hasattr(L, "mmw_factor_random")
    assert L.mmw_factor_random.argtypes == L.mmw_factor_spectral.argtypes
    sig = inspect.signature(_lib.Solver.factor_random).parameters
    assert list(sig) == ["self", "cols", "seed", "resident", "index_order"] and sig["resident"].default is False and sig["index_order"].default is False


@pytest.fixture(scope="module")
def host_handles():
    state = state_from(load_golden("run_env75"))
    hs = [_lib.Solver(4, state, 3, 0.1, dtype=dt, device=-1) for dt in (_lib.F64, _lib.F32)]
    yield hs
    for s in hs:
        s.close()


def test_refusals_name_the_value(host_handles):
    L = _lib.lib()
    out = np.full(80, 7.0)
    assert L.mmw_factor_random(None, 4, 0, _lib._pd(out), 1) == -1 and "mmw_factor_random" in last_error() and "null solver handle" in last_error()
    for s in host_handles:
        for cols in (0, -1, -2 ** 31):
            assert L.mmw_factor_random(s._h, cols, 0, None, 1) == -1
            assert "mmw_factor_random: cols = %d must be >= 1" % cols in last_error()
        for io in (2, -1, 256):
            assert L.mmw_factor_random(s._h, 4, io, None, 1) == -1
            assert "mmw_factor_random: index_order = %d must be 0 or 1" % io in last_error()
        for cols in (MAX_COLS + 1, 2 ** 31 - 1):
            assert L.mmw_factor_random(s._h, cols, 1, None, 1) == -1
            assert "cols = %d exceeds %d" % (cols, MAX_COLS) in last_error()
        # what is in range reaches the handle itself: a device -1 handle has nowhere to draw (MMW_ERR_STATE, as a host-only batch
        # answers mmw_batch_factor_random)
        for cols, io in ((1, 0), (8, 1), (MAX_COLS, 0)):
            assert L.mmw_factor_random(s._h, cols, io, _lib._pd(out) if cols == 1 else None, 1) == -3 and "host-only" in last_error()
        with pytest.raises(_lib.MMWError, match="status -3"):
            s.factor_random(8, 1, resident=True)
        with pytest.raises(_lib.MMWError, match="status -1: mmw_factor_random: cols = 0"):
            s.factor_random(0, 1)
        assert getattr(s, "_last_rank", None) is None and getattr(s, "_factor_serial", 0) == 0  # a refused call leaves the wrapper as it was
    assert np.all(out == 7.0)  # nothing was written


def test_a_host_only_batch_answers_the_same_status():
    state = state_from(load_golden("run_env75"))
    b = _lib.BatchSolver([4], [state], 1, 0.1, device=-1)
    with pytest.raises(_lib.MMWError, match="status -3"):
        b.factor_random([1])
    b.close()


def test_draws_must_be_host_or_device():
    for bad in ("bogus", "", None, "Device"):
        with pytest.raises(ValueError, match="draws must be 'host' or 'device'"):
            rand_sdp_solver(draws=bad)
    sig = inspect.signature(rand_sdp_solver.__init__).parameters
    assert list(sig) == ["self", "nit", "rank_radio", "alpha", "draws", "seed", "device"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("draws", "seed", "device"))
    assert (sig["nit"].default, sig["rank_radio"].default, sig["alpha"].default, sig["draws"].default, sig["seed"].default, sig["device"].default) == (100, 2, 1., "host", 0, 0)
    assert rand_sdp_solver().draws == "host" and rand_sdp_solver(draws="device", seed=5).embedding_key() == probe_seed(5, 0, 0x40000)
    assert spectral_sdp_solver(device=-1).draws == "host"  # (the subclass keeps the class default)


@pytest.mark.parametrize("Z,rank_radio", [(3, 2), (7, 1), (5, 3)])
def test_host_draws_consume_the_global_stream_as_before(Z, rank_radio):
    state = state_from(load_golden("run_env75"))
    K = state[0].shape[0]
    for alg in (rand_sdp_solver(10, rank_radio), rand_sdp_solver(10, rank_radio, draws="host", seed=9, device=3)):
        np.random.seed(123)
        ok, got = alg.run_with_state(0, Z, state)
        after = np.random.random_sample()
        np.random.seed(123)
        want = np.random.randn(K, Z * rank_radio)
        want = want / np.linalg.norm(want, axis=1, keepdims=True)
        assert ok is True and isinstance(got, np.ndarray) and got.tobytes() == want.tobytes()
        assert after == np.random.random_sample()
        assert alg._dev is None  # no handle was made for the draw


def test_device_draws_ask_the_cached_handle_and_no_host_state(monkeypatch):
    """draws="device" on stubs: `run_with_state` takes the handle `_device_solver` caches for the state and asks it for
    factor_random(Z rank_radio, probe_seed(seed, 0, 0x40000), resident, index-ordered); the global stream is not touched and the
    index-ordered block passes through `index_ordered` as it is."""
    asked = []

    class Handle:
        def factor_random(self, cols, seed, resident=False, index_order=False):
            asked.append((cols, seed, resident, index_order))
            df = _lib.DeviceFactor.__new__(_lib.DeviceFactor)
            df._solver, df._serial, df._host, df.index_ordered, df.shape = self, 1, None, True, (9, cols)
            return df

    h = Handle()
    alg = rand_sdp_solver(10, 3, draws="device", seed=5, device=2)
    assert alg._device_index == 2
    monkeypatch.setattr(alg, "_device_solver", lambda Z, state, **k: asked.append(("solver", Z, state)) or h)
    np.random.seed(4)
    nxt = np.random.RandomState(4).random_sample()
    ok, gX = alg.run_with_state(0, 7, "the state")
    assert ok is True and asked == [("solver", 7, "the state"), (21, probe_seed(5, 0, 0x40000), True, True)]
    assert alg.index_ordered(gX) is gX and rand_sdp_solver.index_ordered(gX) is gX and gX._host is None
    assert np.random.random_sample() == nxt
    plain = np.arange(6.0).reshape(3, 2)
    assert np.array_equal(rand_sdp_solver.index_ordered(plain), plain * (1.0 - np.arange(3) * 2.0 ** -32)[:, None])


# ---- the width rule past the sketch's four passes -------------------------------------------------------------------------------------
def lane_rule_block(K, cols, seed):
    """k_factor_random's rule restated: lane l of a row's 64 takes the groups l + 64 i, i = 0, 1, ... while the group exists (as many
    passes as the width needs), adds the squares of its columns < cols in that order, the 64 sums meet pairwise (lanes 32 apart, 16
    apart, then inside a row of 16), every entry is multiplied by 1 / sqrt(sum)."""
    groups = -(-cols // 2)
    w = pr.philox4x32_10(np.arange(K)[:, None], np.arange(groups)[None, :], 0, pr.TAG_SKETCH, seed & 0xFFFFFFFF, seed >> 32)
    n = pr.normals_f64(w).reshape(K, 2 * groups)
    n[:, cols:] = 0.0
    lane = np.zeros((K, 64))
    passes = 0
    for i in range(-(-groups // 64)):
        passes += 1
        for v in range(2):
            c = 2 * (np.arange(64) + 64 * i) + v
            ok = c < 2 * groups
            lane[:, ok] += n[:, c[ok]] ** 2
    s = lane[:, :32] + lane[:, 32:]
    s = s[:, :16] + s[:, 16:]
    ss = s.sum(axis=1)
    return n[:, :cols] * (1.0 / np.sqrt(ss))[:, None], passes


@pytest.mark.parametrize("cols", [512, 513, 1030, 1537])
def test_the_width_rule_past_512_columns_is_the_restatements(cols):
    """Every group p < ceil(cols / 2) belongs to exactly one (lane, pass) -- lane p % 64, pass p // 64 -- whatever the width, so the
    rule draws `philox_ref._draw`'s columns, no more and no fewer, and its norm is `philox_ref.sketch`'s to summation order
    (<= cols eps / 2 relative on the sum)."""
    seed = (1 << 32) + 1
    groups = -(-cols // 2)
    owners = np.zeros(groups, dtype=np.int64)
    for lane in range(64):
        p = lane
        while p < groups:
            owners[p] += 1
            p += 64
    assert np.all(owners == 1)
    got, passes = lane_rule_block(5, cols, seed)
    assert passes == -(-groups // 64) and (passes > 4) == (cols > 512)
    ref = pr.sketch(5, cols, seed, 0, "f64")
    assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 1e-15
    assert np.max(np.abs(np.linalg.norm(got, axis=1) - 1.0)) <= 1e-15
    # a column past `cols` must not count: with it the norm is off by far more than rounding
    if cols % 2:
        w = pr.philox4x32_10(np.arange(5)[:, None], np.array([[groups - 1]]), 0, pr.TAG_SKETCH, seed & 0xFFFFFFFF, seed >> 32)
        extra = pr.normals_f64(w)[:, 0, 1]
        assert np.min(np.abs(extra)) > 1e-3
