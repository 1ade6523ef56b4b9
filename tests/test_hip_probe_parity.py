"""Oracle parity of the trajectories the colouring and the ER configurations really run.

test_hip_timed_path.py holds the benchmark's 48-iteration fast path to the CPU oracle.  The paths here go further:

* the probes of a bisection (`binary_search.py` -> `mmw._run`): 150 iterations in ONE `mmw_iterate` call on a handle that
  `mmw_set_slots` rebinds from probe to probe, at slot counts where the matrix grows fast enough for chunks to be discarded
  and tried again (`settle` in csrc/solver.h), and the probe after such a probe, which runs with `replays > 0`;
* the cautious second attempt at a discarded chunk and the synchronous replay behind it, each forced;
* er-5pct-2k (fp64 and fp32) and er-50k on the chunked device-RNG path, and er-50k's synchronous path.

The device draws its sketches; `mmw_sketch` regenerates the Philox block of any (seed, iteration) and the oracle follows the
same run on them.  Bars (north star): exp(L/2)R <= 1e-5 relative Frobenius, every other field <= 1e-4 (fp32), <= 1e-8 (fp64).
Every test also asserts, from the handle's counters and the `MMW_VERBOSE` lines, that the path it targets did run.
"""
import re

import numpy as np
import pytest

from conftest import relerr
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.graphs import er_contention_graph, journal_graph
from test_hip_timed_path import compare, compare_calls, oracle_for, run_calls, snapshot

pytestmark = pytest.mark.gpu

F32_BARS, F64_BARS = (1e-5, 1e-4), (1e-8, 1e-8)
_REPLAY = re.compile(r"\[replay\] iterations (\d+)\.\.(\d+) \(Z (\d+)\) ([a-z ]+): reason bits (\d+)")


def replay_lines(err):
    """(first, last, Z, what, reason bits) of every `[replay]` line MMW_VERBOSE printed."""
    return [(int(a), int(b), int(z), how, int(bits)) for a, b, z, how, bits in _REPLAY.findall(err)]


def counters(s):
    """(F_DUAL_INFO, replays): both count from mmw_create, so a probe's share is a difference."""
    s.sync()
    return s.read(_lib.F_DUAL_INFO).copy(), int(s.read(_lib.F_BLOCKING)[3])


# The first probe of the benchmark's colouring (journal-1pct) is Z = 186; the converged colouring is decided at Z ~ 35..45.
# Probe seeds of mmw._run are (seed << 20) + run; any fixed seed is one probe.
PROBE_SEEDS = {186: 1, 35: 2, 41: 3}


@pytest.mark.timeout(1500)
def test_colouring_probes_on_a_reused_handle_meet_the_oracle(monkeypatch, capfd):
    """journal-1pct, fp32, device RNG, eta 0.04, nit 150, on ONE handle: the first midpoint (Z = 186) brings the handle into the
    state a search leaves it in; then Z = 35 as one 150-iteration call (as mmw._run makes it, read at its end) and Z = 41, which
    starts with replays > 0, in two calls of 75.  DESIGN (the colouring table and the cautious second attempt) names Z = 35 as a
    probe whose chunks are discarded; the counters and the verbose lines show that the two probes took the first-order form in
    one fp16 half and in hi + lo, Lanczos steps, discarded chunks and a cautious attempt.  The Z = 41 probe continues down the
    pipeline: its rank-80 factor against svds of the oracle's average, and one rounding batch on that factor, exactly.

    With these seeds MMW_VERBOSE shows, at Z = 35, iterations 8..39 discarded (reason bits 48: the 16-bit operand gate and the
    first-order certificate) and 40..71 discarded (bit 2: a lagged plan), each followed by an accepted cautious attempt; at
    Z = 41, iterations 107..138 discarded (bit 2), cautious attempt accepted.  A full bisection of this instance probes
    186, 105, 65, 45, 35, 40, 43, 42, 41 and discards chunks at 35, 40 and 42."""
    state = journal_graph(28, 0.0319, 0)
    eta, nit = 0.04, 150
    s = _lib.Solver(186, state, nit, eta, dtype=_lib.F32)
    s.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6)  # mmw(dtype="f32") defaults, as bench.py's colouring runs them
    s.set_timing(8)
    s.iterate(nit, None, PROBE_SEEDS[186])
    c_start = counters(s)
    monkeypatch.setenv("MMW_VERBOSE", "1")
    capfd.readouterr()

    # probe Z = 35: one call of 150
    Z1 = 35
    s.set_slots(Z1, nit)
    s.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6)
    s.set_timing(8)
    (got1,) = run_calls(s, [nit], PROBE_SEEDS[Z1])
    c1 = counters(s)
    lines1 = replay_lines(capfd.readouterr().err)
    # its sketches from a second handle at the same slot count (the first moves on to Z = 41)
    sk = _lib.Solver(Z1, state, 1, eta, dtype=_lib.F32)
    assert np.array_equal(sk.sketch(PROBE_SEEDS[Z1], nit - 1), s.read(_lib.F_SKETCH))

    # probe Z = 41: two calls of 75, on a handle that has replayed chunks
    Z2 = 41
    assert c1[1] > 0, (c_start, c1, lines1)
    s.set_slots(Z2, nit)
    s.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6)
    s.set_timing(8)
    got2 = run_calls(s, [75, 75], PROBE_SEEDS[Z2])
    c2 = counters(s)
    lines2 = replay_lines(capfd.readouterr().err)
    monkeypatch.delenv("MMW_VERBOSE")

    # the regime: deltas over the two probes (n = 300 iterations)
    d = c2[0] - c_start[0]
    lines = lines1 + lines2
    why = (d, c_start, c1, c2, lines)
    assert d[3] >= 1, why                # first-order products with the matrix in one fp16 half
    assert d[2] - d[3] >= 1, why         # first-order products in hi + lo
    assert 2 * nit - d[2] >= 1, why      # Lanczos steps
    assert any(w == "discarded" for *_, w, _b in lines), why
    assert any(w.startswith("cautious attempt") for *_, w, _b in lines), why
    assert c2[1] > c_start[1], why

    # rank-80 factor and one rounding batch of the Z = 41 probe (the factor stays on the device for the rounding)
    rank = min(s.K - 1, 2 * (Z2 - 1))
    assert rank == 80
    gX = s.factor(rank, seed=2, resident=True)
    rng = np.random.default_rng(11)
    rv = rng.standard_normal((2, Z2, rank))
    rv /= np.linalg.norm(rv, axis=2, keepdims=True)
    z, rem = s.round(Z2, gX, rv)
    X = np.array(gX)

    o1 = oracle_for(sk.sketch, state, Z1, nit, eta, PROBE_SEEDS[Z1], [nit])
    compare(got1, o1, 0, True, nit)
    del o1
    o2 = oracle_for(s.sketch, state, Z2, nit, eta, PROBE_SEEDS[Z2], [75, 75])
    compare_calls(got2, o2, nit)

    ref = orc.factor_xavg(o2.pattern.csr(o2.xavg), rank)
    rows = np.random.default_rng(0).choice(s.K, size=512, replace=False)
    assert relerr(X[rows] @ X.T, ref[rows] @ ref.T) < 1e-4
    for b in range(rv.shape[0]):
        z_ref, _, rem_ref, un = orc.rounding_one_attempt(Z2, X, state, rv[b], randint=lambda Z_, size: np.zeros(size))
        assert int(rem[b]) == rem_ref
        assert np.array_equal(z[b] < 0, un)
        assert np.array_equal(z[b][~un], z_ref[~un].astype(np.int32))
    sk.close()
    s.close()


@pytest.mark.timeout(600)
def test_cautious_attempt_and_synchronous_replay_meet_the_oracle(monkeypatch, capfd):
    """The settings of test_first_order_certificate_counts_the_fp16_rounding (MMW_FV_DU_SCALE=200 makes the first-order certificate
    miss).  Two handles on the same seed: the default one discards the chunk and accepts its cautious second attempt; one with
    MMW_CAUTIOUS_REPLAY=0 discards it and replays it synchronously.  Both against the oracle at every field, mid-run and at the end."""
    state = journal_graph(16, 0.02, seed=4)
    Z, nit, eta, seed = 24, 48, 0.01, 9
    calls = [24, 24]
    monkeypatch.setenv("MMW_FV_DU_SCALE", "200")  # (read at mmw_create, like MMW_CAUTIOUS_REPLAY)
    monkeypatch.setenv("MMW_VERBOSE", "1")
    runs = {}
    for mode in ("cautious", "synchronous"):
        if mode == "synchronous":
            monkeypatch.setenv("MMW_CAUTIOUS_REPLAY", "0")
        capfd.readouterr()
        s = _lib.Solver(Z, state, nit, eta, dtype=_lib.F32)
        s.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6)
        snaps = run_calls(s, calls, seed)
        info, replays = counters(s)
        runs[mode] = (snaps, info, replays, replay_lines(capfd.readouterr().err))
        if mode == "cautious":
            o = oracle_for(s.sketch, state, Z, nit, eta, seed, calls)
        s.close()
    for mode, (snaps, info, replays, lines) in runs.items():
        what = [w for *_, w, _b in lines]
        assert info[2] > 0 and replays >= 1, (mode, info, replays, lines)
        assert any(w == "discarded" and bits & 32 for *_, w, bits in lines), (mode, lines)  # the first-order certificate missed
        if mode == "cautious":
            assert "cautious attempt accepted" in what and "replayed synchronously" not in what, lines
        else:
            assert "replayed synchronously" in what and not any(w.startswith("cautious") for w in what), lines
        compare_calls(snaps, o, nit)


def _generic_path_asserts(s, info):
    assert int(s.read(_lib.F_SPMM_KIND)[0]) == 0  # no locality: the generic CSR SpMM
    assert info[1] > 0, info                        # the softmax ran inside the violation pass


@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype,bars", [(_lib.F64, F64_BARS), (_lib.F32, F32_BARS)], ids=["f64", "f32"])
def test_er_5pct_2k_chunked_device_rng_meets_the_oracle(dtype, bars):
    """configs[1] (N = 2000, 5 % ER, Z = 32) on the path the benchmark times: chunks without readbacks, device RNG, lagged plans,
    the fused softmax; 40 iterations in two calls of 20, compared at iterations 19 and 39 (its synchronous path is in
    test_hip_configs.py)."""
    state = er_contention_graph(2000, 0.05, 0)
    Z, nit, eta, seed, calls = 32, 40, 0.04, 31, [20, 20]
    s = _lib.Solver(Z, state, nit, eta, dtype=dtype)
    s.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6 if dtype == _lib.F32 else 1e-12)
    snaps = run_calls(s, calls, seed)
    info, _ = counters(s)
    _generic_path_asserts(s, info)
    o = oracle_for(s.sketch, state, Z, nit, eta, seed, calls)
    s.close()
    compare_calls(snaps, o, nit, bars)


@pytest.mark.timeout(1200)
def test_er_50k_synchronous_and_chunked_paths_meet_the_oracle(monkeypatch, capfd):
    """configs[4] (N = 50 000, 0.2 % ER, Z = 32, fp32), one oracle run of 24 iterations on the device's sketches of one seed.
    Handle 1: the first 3 iterations one at a time on uploaded sketches (the synchronous path), every field at every iteration.
    Handle 2: 24 iterations as two calls of 12 on the device-RNG path, compared at iterations 11 and 23.  Whether a lagged plan
    missed in this window (reason bit 2 in the MMW_VERBOSE lines) is printed, not asserted: with seed 5 none did and no chunk was
    discarded (the misses DESIGN reports for er-50k come later in a run)."""
    state = er_contention_graph(50000, 0.002, 0)
    Z, nit, eta, seed, calls = 32, 24, 0.04, 5, [12, 12]
    monkeypatch.setenv("MMW_VERBOSE", "1")
    capfd.readouterr()
    b = _lib.Solver(Z, state, nit, eta, dtype=_lib.F32)
    b.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6)
    chunked = run_calls(b, calls, seed)
    info, replays = counters(b)
    lines = replay_lines(capfd.readouterr().err)
    monkeypatch.delenv("MMW_VERBOSE")
    _generic_path_asserts(b, info)
    with capfd.disabled():
        print("\n[er-50k] dual info %s, replays %d, lagged plan missed: %s, replay lines %s"
              % (info.tolist(), replays, any(bits & 2 for *_, bits in lines), lines))

    a = _lib.Solver(Z, state, nit, eta, dtype=_lib.F32)
    a.set_expm(_lib.EXPM_LANCZOS, 12, 1e-6)
    sync = []
    for i in range(3):
        a.iterate(1, b.sketch(seed, i))
        sync.append(snapshot(a))
    a.close()

    o = orc.MMWOracle(nit=nit, eta=eta)
    o.run(Z, state, lambda i, K, D: b.sketch(seed, i), keep_trace={0, 1, 2, 11, 23}, factor=False)
    b.close()
    for i, got in enumerate(sync):
        compare(got, o, i, False, nit)
    compare(chunked[0], o, 3, False, nit)
    compare(chunked[1], o, 4, True, nit)
