"""GPU checks of the carry across states on the solver handle (mmw_carry, csrc/solver_carry.h, csrc/kernels_carry.h) and of the re-solve
workflow built on it (`online.online_resolve_sweep`).

The state pairs are those of tests/test_carry_handle_host.py: carry_oracle's (a) mobile_drop(5, 75e-4, 3) before and after one second at
3 m/s, (b) the hand-made K = 4 pair whose L patterns share only the diagonal, (c) K = 2 losing / gaining its one association pair,
(k192_moved), and the drops of tests/helpers/online_cases.py moved the same way (k1083: rows longer than a wavefront).  In every moved
pair the gained association pairs are stored in the old pattern as GAIN entries -- L and X carry a value there, the pair's Y and
e_accu carry 0 -- and pair (b) gains pairs whose entry the old pattern lacks altogether (asserted on the CPU in the host file).
Bars: bitwise wherever two handles, or a handle and a gather, are compared; against the CPU restatement (carry_oracle.run) 1e-9
relative in fp64 at set_expm(16, 1e-13) (the bar of test_hip_batch_carry.py and test_hip_loop.py), and in fp32 on device sketches the
bars of test_hip_probe_parity.py: exp(L/2)R <= 1e-5, every other field <= 1e-4."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import carry_oracle  # noqa: E402
import online_cases as OC  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch, online  # noqa: E402
from sig_sdp_mmw_amd.batch import probe_seed  # noqa: E402
from sig_sdp_mmw_amd.mmw import factor_rank_seed  # noqa: E402

pytestmark = pytest.mark.gpu

ETA = 0.05
DTYPES = [_lib.F64, _lib.F32]
ITERATE = ("F_Y", "F_E_ACCU", "F_LVAL", "F_XVAL", "F_XAVG", "F_YAVG")  # the iterate and its sums
AFTER = ITERATE + ("F_E_THIS", "F_XHALF", "F_EXPM_INFO")  # ... and what an iteration leaves beside them
ON_L = ("F_LVAL", "F_XVAL", "F_XAVG")
# carried field -> the source field it is gathered from (the sums restart from the carried X / Y)
CARRIED = {"F_LVAL": "F_LVAL", "F_XVAL": "F_XVAL", "F_XAVG": "F_XVAL", "F_Y": "F_Y", "F_YAVG": "F_Y", "F_E_ACCU": "F_E_ACCU"}


@functools.lru_cache(maxsize=None)
def pairs():
    """name -> (old state, new state, Z old, Z new)"""
    out = {"a": carry_oracle.moved_pair(5, carry_oracle.PAIR_A_SEED) + (6, 7), "b": carry_oracle.pair_b() + (2, 3),
           "c_lose": carry_oracle.pair_c("lose") + (2, 2), "c_gain": carry_oracle.pair_c("gain") + (2, 2),
           "k192_moved": carry_oracle.moved_pair(8, 2) + (10, 9)}
    for n in OC.NAMES:
        Z = OC.CASES[n][3]
        out[n] = (OC.host_state(n, 0), OC.host_state(n, 1), Z, Z)
    return out


FIVE = ("a", "b", "c_lose", "c_gain", "k192_moved")


def read(s, names):
    return {f: s.read(getattr(_lib, f)) for f in names}


def same(got, ref, what):
    assert set(got) == set(ref)
    for f in ref:
        assert got[f].shape == ref[f].shape and np.array_equal(got[f], ref[f]), (what, f)


def last_error():
    return _lib.lib().mmw_last_error().decode()


# ---- 1. what is written, and what is not ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FIVE + ("k1083",))
def test_carried_fields_are_the_mapped_source_and_the_source_is_untouched(name, dtype):
    old, new, zo, zn = pairs()[name]
    seed = 41
    src, twin = (_lib.Solver(zo, old, 5, ETA, dtype=dtype) for _ in range(2))
    dst = _lib.Solver(zn, new, 4, ETA, dtype=dtype)
    src.iterate(3, None, seed=seed)  # (device sketches: the chunk is still pending when the carry comes)
    twin.iterate(3, None, seed=seed)
    dst.carry_from(src)
    assert dst.iterations_done == 0
    have = read(twin, AFTER)  # what the source held: its twin was never carried from
    same(read(src, AFTER), have, "source after the carry")
    rl, rc = carry_oracle.maps(orc.Pattern(zo, old), orc.Pattern(zn, new))
    ml, mc = dst.carry_map(src)
    got = read(dst, AFTER)
    for f, frm in CARRIED.items():
        for how, (l, c) in (("helper", (rl, rc)), ("carry_map", (ml.astype(np.int64), mc.astype(np.int64)))):
            assert np.array_equal(got[f], carry_oracle.gather(have[frm], l if f in ON_L else c)), (f, how)
    assert np.array_equal(got["F_XAVG"], got["F_XVAL"]) and np.array_equal(got["F_YAVG"], got["F_Y"])
    for f in ("F_E_THIS", "F_XHALF", "F_EXPM_INFO"):
        assert not np.any(got[f]), f
    assert np.any(got["F_LVAL"]) and np.any(got["F_E_ACCU"]) and np.any(got["F_XVAL"])  # (something was there to carry)
    assert dst.iterations_done == 0
    dst.iterate(4, None, seed=seed + 1)  # it runs the iterations it announced, no more
    dst.sync()
    assert dst.iterations_done == 4 and all(np.all(np.isfinite(v)) for v in read(dst, AFTER).values())
    with pytest.raises(_lib.MMWError, match="more iterations than announced"):
        dst.iterate(1, None, seed=seed + 1)
    src.iterate(2, None, seed=seed)  # and the source continues as if nobody had read it
    twin.iterate(2, None, seed=seed)
    same(read(src, AFTER), read(twin, AFTER), "source continued")
    for h in (src, twin, dst):
        h.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_source_may_continue_the_moment_the_carry_returns(dtype):
    """k1083: `src.iterate` straight after `carry_from`, with no read or sync of the destination in between.  The gather runs on the
    destination's stream and reads the source's buffers, which the source's next DUAL and LOSS passes rewrite: `mmw_carry` returns only
    after it, so the destination holds the gather of what the source held AT the carry (its twin, stopped there) and the source
    continues like the twin."""
    old, new, zo, zn = pairs()["k1083"]
    seed = 43
    src, twin = (_lib.Solver(zo, old, 11, ETA, dtype=dtype) for _ in range(2))
    dst = _lib.Solver(zn, new, 4, ETA, dtype=dtype)
    src.iterate(3, None, seed=seed)
    twin.iterate(3, None, seed=seed)
    dst.carry_from(src)
    src.iterate(8, None, seed=seed)  # (enqueued at once: nothing has looked at dst)
    have = read(twin, ITERATE)
    got = read(dst, ITERATE)
    rl, rc = carry_oracle.maps(orc.Pattern(zo, old), orc.Pattern(zn, new))
    for f, frm in CARRIED.items():
        assert np.array_equal(got[f], carry_oracle.gather(have[frm], rl if f in ON_L else rc)), f
    twin.iterate(8, None, seed=seed)
    same(read(src, AFTER), read(twin, AFTER), "source continued at once")
    for h in (src, twin, dst):
        h.close()


# ---- 2. on one state the carry is the warm slot change ----------------------------------------------------------------------------------
SAME_STATE = {"a": ("a", 6, 7), "k192": ("k192_moved", 10, 9), "b": ("b", 2, 3)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("leg", ["uploaded", "device"])
@pytest.mark.parametrize("name", list(SAME_STATE))
def test_carry_onto_the_same_state_is_the_warm_slot_change(name, leg, dtype):
    """dst on the same state at Z2, carried, against src.set_slots(Z2, n, warm=True): the iterate and its sums before the iterations,
    everything after them.  On device sketches n = 24 is several chunks, the first capped at 8 (ChunkPolicy::warm_fresh): only a
    destination that took the run history over completely launches them as the slot change does."""
    pair, Z1, Z2 = SAME_STATE[name]
    state = pairs()[pair][0]
    K = state[0].shape[0]
    n1, n = (4, 3) if leg == "uploaded" else (10, 24)
    rng = np.random.default_rng(5)
    sk1 = np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * Z1))) for _ in range(n1)]) if leg == "uploaded" else None
    sk2 = np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * Z2))) for _ in range(n)]) if leg == "uploaded" else None
    src = _lib.Solver(Z1, state, n1, ETA, dtype=dtype)
    src.iterate(n1, sk1, seed=7)
    dst = _lib.Solver(Z2, state, n, ETA, dtype=dtype)
    dst.carry_from(src)
    src.set_slots(Z2, n, warm=True)
    same(read(dst, ITERATE), read(src, ITERATE), "before")
    assert dst.iterations_done == src.iterations_done == 0
    src.iterate(n, sk2, seed=8)
    dst.iterate(n, sk2, seed=8)
    same(read(dst, AFTER), read(src, AFTER), "after")
    assert np.array_equal(dst.read(_lib.F_BLOCKING), src.read(_lib.F_BLOCKING))  # (the replays counted so far came along)
    src.close()
    dst.close()


# ---- 3. across states against the CPU restatement ---------------------------------------------------------------------------------------
def against_oracle(got, w, bars):
    errs = {k: relerr(got[k], w[k]) for k in got}
    print({k: "%.2e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= (bars[0] if k == "X_half" else bars[1]), (k, v)


def final(dst):
    return {"lval": dst.read(_lib.F_LVAL), "xval": dst.read(_lib.F_XVAL), "Y": dst.read(_lib.F_Y), "e_accu": dst.read(_lib.F_E_ACCU),
            "xsum": dst.read(_lib.F_XAVG), "ysum": dst.read(_lib.F_YAVG), "X_half": dst.read(_lib.F_XHALF)}


@pytest.mark.parametrize("name", ["a", "k192_moved"])
def test_carry_across_states_follows_the_oracle_fp64(name):
    """5 iterations, the carry, 4 iterations on uploaded sketches.  After all announced iterations the handle's sums hold the carried
    X / Y and the n2 - 1 new terms the oracle's hold (tests/helpers/warm_oracle.py on the two conventions)."""
    old, new, zo, zn = pairs()[name]
    K, n1, n2 = old[0].shape[0], 5, 4
    rng = np.random.default_rng(11)
    sk1 = np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * zo))) for _ in range(n1)])
    sk2 = np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * zn))) for _ in range(n2)])
    src = _lib.Solver(zo, old, n1, ETA, dtype=_lib.F64)
    src.set_expm(_lib.EXPM_LANCZOS, 16, 1e-13)
    src.iterate(n1, sk1)
    dst = _lib.Solver(zn, new, n2, ETA, dtype=_lib.F64)
    dst.set_expm(_lib.EXPM_LANCZOS, 16, 1e-13)
    dst.carry_from(src)
    dst.iterate(n2, sk2)
    w = carry_oracle.run(zo, n1, old, zn, n2, new, ETA, lambda it, K_, D: sk1[it], lambda it, K_, D: sk2[it])
    against_oracle(final(dst), w, (1e-9, 1e-9))
    src.close()
    dst.close()


@pytest.mark.parametrize("name", ["a", "k192_moved"])
def test_carry_across_states_follows_the_oracle_fp32(name):
    """12 + 10 iterations on device sketches (chunks without readback on both sides of the carry), the oracle following on
    `Solver.sketch`'s blocks."""
    old, new, zo, zn = pairs()[name]
    n1, n2, seed1, seed2 = 12, 10, 21, 22
    src = _lib.Solver(zo, old, n1, ETA, dtype=_lib.F32)
    src.iterate(n1, None, seed=seed1)
    dst = _lib.Solver(zn, new, n2, ETA, dtype=_lib.F32)
    dst.carry_from(src)
    dst.iterate(n2, None, seed=seed2)
    got = final(dst)
    w = carry_oracle.run(zo, n1, old, zn, n2, new, ETA, lambda it, K_, D: src.sketch(seed1, it), lambda it, K_, D: dst.sketch(seed2, it))
    against_oracle(got, w, (1e-5, 1e-4))
    src.close()
    dst.close()


# ---- 4. where the destination came from does not matter ---------------------------------------------------------------------------------
def env_at(name, moved):
    ap, p0, p1 = OC.positions(name)
    return online._env(type("D", (), {"sta_locs": p1 if moved else p0, "ap_locs": ap})(), 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_destinations_origin_does_not_matter(dtype, monkeypatch):
    """mmw_create on the moved environment's arrays, mmw_create_from_env and mmw_create_from_csr: carried from one source they hold the
    same bits, and -- the generator's handle on the pattern-only blocking of the other two (MMW_ENV_RCM=1) -- still do after iterating.
    A source that never iterated leaves the destination a fresh handle."""
    name, n = "k75", 6
    Z = OC.CASES[name][3]
    env = env_at(name, 0)
    src = _lib.Solver.from_env(env, Z, 5, ETA, dtype=dtype)
    idle = _lib.Solver.from_env(env, Z, 5, ETA, dtype=dtype)
    src.iterate(5, None, seed=3)
    env.move(OC.positions(name)[2])
    state = env.state()
    csr = _lib.DeviceCSR.upload(state)
    monkeypatch.setenv("MMW_ENV_RCM", "1")

    def three():
        return [_lib.Solver(Z, state, n, ETA, dtype=dtype), _lib.Solver.from_env(env, Z, n, ETA, dtype=dtype), _lib.Solver.from_csr(csr, Z, n, ETA, dtype=dtype)]

    dsts, cold, fresh = three(), three(), three()
    monkeypatch.delenv("MMW_ENV_RCM")
    spatial = _lib.Solver.from_env(env, Z, n, ETA, dtype=dtype)  # the generator's handle on its own row blocks
    for d in dsts + [spatial]:
        d.carry_from(src)
    for d in cold:
        d.carry_from(idle)
    ref = read(dsts[0], ITERATE)
    assert np.any(ref["F_LVAL"])
    # mmw_carry_map on handles built on the device (their lists are fetched first), against the host-built handle's and the helper's
    want_l, want_c = carry_oracle.maps(orc.Pattern(Z, OC.host_state(name, 0)), orc.Pattern(Z, state))
    for d in dsts + [spatial]:
        ml, mc = d.carry_map(src)
        assert np.array_equal(ml, want_l) and np.array_equal(mc, want_c)
    for d in dsts[1:] + [spatial]:
        same(read(d, ITERATE), ref, "before")
    for d, f in zip(cold, fresh):
        same(read(d, AFTER), read(f, AFTER), "a source that never iterated")
    for d in dsts + cold + fresh:
        d.iterate(n, None, seed=4)
    ref = read(dsts[0], AFTER)
    assert not np.array_equal(ref["F_LVAL"], read(fresh[0], AFTER)["F_LVAL"])
    for d in dsts[1:]:
        same(read(d, AFTER), ref, "after")
    for d, f in zip(cold, fresh):
        same(read(d, AFTER), read(f, AFTER), "cold after")
    for h in dsts + cold + fresh + [spatial, src, idle, csr, env]:
        h.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_handles_alone():
    old, new, zo, zn = pairs()["a"]
    src = _lib.Solver(zo, old, 4, ETA, dtype=_lib.F64)
    src.iterate(4, None, seed=2)
    dst = _lib.Solver(zn, new, 3, ETA, dtype=_lib.F64)
    before = read(src, AFTER), read(dst, AFTER)
    L = _lib.lib()

    def refused(d, s, status, *texts):
        rc = L.mmw_carry(d._h if d is not None else None, s._h if s is not None else None)
        msg = last_error()
        assert rc == status and all(t in msg for t in texts), (rc, msg)

    refused(None, src, -1, "null solver handle")
    refused(dst, None, -1, "null solver handle")
    refused(dst, dst, -1, "mmw_carry", "cannot carry from itself")
    host = _lib.Solver(zn, new, 3, ETA, dtype=_lib.F64, device=-1)
    refused(host, src, -3, "mmw_carry", "host-only handle")
    refused(dst, host, -3, "mmw_carry", "host-only handle")
    single = _lib.Solver(zn, new, 3, ETA, dtype=_lib.F32)
    refused(single, src, -1, "mmw_carry", "fp64 handle", "fp32")
    refused(dst, single, -1, "mmw_carry", "fp32 handle", "fp64")
    small = _lib.Solver(2, pairs()["b"][1], 3, ETA, dtype=_lib.F64)
    refused(small, src, -1, "mmw_carry", "K = 4 here", "K = 75 in the source")
    refused(dst, small, -1, "mmw_carry", "K = 75 here", "K = 4 in the source")
    ran = _lib.Solver(zn, new, 3, ETA, dtype=_lib.F64)
    ran.iterate(2, None, seed=1)
    held = read(ran, AFTER)
    refused(ran, src, -3, "mmw_carry", "has run 2 iterations")
    same(read(ran, AFTER), held, "a destination that has iterated")
    if _lib.device_count() > 1:  # a handle on another device needs a second device to exist
        far = _lib.Solver(zn, new, 3, ETA, dtype=_lib.F64, device=1)
        refused(far, src, -1, "mmw_carry", "device 0", "device 1")
        far.close()
    same(read(src, AFTER), before[0], "source")
    same(read(dst, AFTER), before[1], "destination")
    assert dst.iterations_done == 0 and src.iterations_done == 4
    dst.carry_from(src)  # a served call follows
    assert np.any(dst.read(_lib.F_LVAL)) and dst.iterations_done == 0
    dst.iterate(3, None, seed=1)
    for h in (src, dst, host, single, small, ran):
        h.close()


# ---- 6. the workflow --------------------------------------------------------------------------------------------------------------------
def by_hand(name, n_points, nit, n_p, carry, seed, natt, dtype):
    """The documented steps of online_resolve_sweep, composed here from the public pieces."""
    drop = OC.drop(name)
    env, alg, solver, Z, gX = online._setup(drop, nit, 0.04, seed, 2, 0, dtype)
    out, prev = [], None
    try:
        for p in range(n_points):
            env.move(drop.sta_locs)
            if p:
                s = _lib.Solver.from_env(env, Z, n_p, 0.04, rank_radio=2, dtype=dtype)
                if carry:
                    s.carry_from(solver)
                key = probe_seed(seed, 0, 0xC0000 | p)
                s.iterate(n_p, None, seed=key)
                rank, fseed = factor_rank_seed(drop.K, Z, 2, key)
                assert (rank, fseed) == (min(drop.K - 1, (Z - 1) * 2), key)
                gX = s.factor(rank, seed=fseed, resident=True)
                if prev is not None:
                    prev.close()
                prev = solver = s
            z_vec, rem = online.round_point(solver, env, Z, gX, natt, np.random.default_rng(probe_seed(seed, 0, 0x80000 | p)))
            _, bler = env.evaluate(z_vec, Z)
            out.append((z_vec, rem, bler))
            drop.step_time(1e6, 3.0, 1e5)
    finally:
        if prev is not None:
            prev.close()
        alg.close()
        env.close()
    return Z, out


def check_sweep(name, n_points, nit, carry, dtype=_lib.F32):
    seed, natt = 3, 4
    n_p = batch.warm_iterations(nit, 1.0 / 3.0) if carry else nit
    np.random.seed(1)
    timings = []
    out = online.online_resolve_sweep(OC.drop(name), n_points=n_points, mob_spd_meter_s=3.0, nit=nit, seed=seed, nattempt=natt, dtype=dtype, carry=carry, timings=timings)
    np.random.seed(1)
    Z, want = by_hand(name, n_points, nit, n_p, carry, seed, natt, dtype)
    K = OC.CASES[name][2]
    assert out["Z"] == Z and out["iters"] == [nit] + [n_p] * (n_points - 1) and out["z_vec"].shape == out["bler"].shape == (n_points, K)
    for p, (z_vec, rem, bler) in enumerate(want):
        assert np.array_equal(out["z_vec"][p], z_vec) and out["remainder"][p] == rem and out["bler"][p].tobytes() == bler.tobytes(), p
    assert np.all((0 <= out["z_vec"]) & (out["z_vec"] < Z)) and np.all((0 <= out["bler"]) & (out["bler"] <= 1))
    keys = {"create_s", "carry_s", "iterate_s", "epilogue_s", "evaluate_s", "step_s"}
    assert len(timings) == n_points and all(set(t) == keys and min(t.values()) >= 0.0 for t in timings)
    return out


@pytest.mark.parametrize("carry", [True, False])
def test_online_resolve_sweep_is_its_documented_steps(carry):
    nit = 20
    out = check_sweep("k75", 3, nit, carry)
    assert out["iters"] == [20, 7, 7] if carry else out["iters"] == [20, 20, 20]
    np.random.seed(1)
    once = online.online_sweep(OC.drop("k75"), n_points=1, mob_spd_meter_s=3.0, nit=nit, seed=3, nattempt=4)  # point 0 is online_sweep's
    assert once["Z"] == out["Z"] and np.array_equal(once["z_vec"][0], out["z_vec"][0]) and once["bler"][0].tobytes() == out["bler"][0].tobytes()
    assert once["remainder"][0] == out["remainder"][0]


def test_the_resolve_sweep_above_the_batch_limit():
    assert OC.CASES["k1083"][2] > _lib.BATCH_EPILOGUE_MAX_K
    check_sweep("k1083", 2, 12, True)
