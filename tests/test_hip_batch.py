"""GPU checks of the batched solver (one workgroup per instance, csrc/kernels_batch.h) against the reference's golden vectors,
the CPU oracle and the per-handle path."""
import numpy as np
import pytest
import scipy.sparse

from conftest import RUN_CASES, csr_from, load_golden, relerr, state_from
from oracle import mmw_oracle as orc
from sig_sdp_mmw_amd import _lib

pytestmark = pytest.mark.gpu


def pattern_csr(b, i, vals):
    K = b.sizes[i]["K"]
    return scipy.sparse.csr_matrix((vals, b.read_i32(i, _lib.I_L_INDICES), b.read_i32(i, _lib.I_L_INDPTR)), shape=(K, K))


def sweep_states(cells=(5, 7, 9, 11, 13, 15), seeds=(0,)):
    from sig_sdp_mmw_amd.graphs import journal_graph
    return [journal_graph(c, 75e-4, seed=s) for c in cells for s in seeds]


def test_golden_runs_as_one_batch():
    gs = [load_golden("run_" + n) for n in RUN_CASES]
    states = [state_from(g) for g in gs]
    nits = [int(g["nit"]) for g in gs]
    b = _lib.BatchSolver([int(g["Z"]) for g in gs], states, nits, 0.1)
    b.set_eta([float(g["eta"]) for g in gs])
    b.set_expm(16, 1e-13)
    for i in range(max(nits)):
        b.iterate(1, [g["randv"][i:i + 1] if i < int(g["nit"]) else None for g in gs])
        for j, (name, g) in enumerate(zip(RUN_CASES, gs)):
            if i >= nits[j]:
                continue
            diag = b.read_i32(j, _lib.I_DIAG_POS)
            assert relerr(b.read(j, _lib.F_E_THIS), g["e_this"][i]) < 1e-9, (name, i)
            assert relerr(b.read(j, _lib.F_E_ACCU), g["e_accu"][i]) < 1e-9, (name, i)
            assert relerr(b.read(j, _lib.F_Y), g["Y"][i]) < 1e-9, (name, i)
            L = pattern_csr(b, j, b.read(j, _lib.F_LVAL))
            Lref = csr_from(g, "Laccu%d" % i)
            assert abs(L - Lref).max() < 1e-10 * max(1e-3, abs(Lref).max()), (name, i)
            assert relerr(b.read(j, _lib.F_XHALF), g["X_half_it"][i]) < 1e-9, (name, i)
            xv = b.read(j, _lib.F_XVAL)
            assert relerr(xv[diag], g["X_mdiag"][i]) < 1e-9, (name, i)
            xo = xv.copy()
            xo[diag] = 0
            assert abs(pattern_csr(b, j, xo) - csr_from(g, "Xoffdi%d" % i)).max() < 1e-9, (name, i)
    for j, (name, g) in enumerate(zip(RUN_CASES, gs)):
        assert b.iterations_done(j) == nits[j]
        xavg = pattern_csr(b, j, b.read(j, _lib.F_XAVG) / nits[j])
        assert abs(xavg - csr_from(g, "Xavgd")).max() < 1e-9, name
    with pytest.raises(_lib.MMWError):
        b.iterate(1, [None] * len(gs))  # every instance has run its nit
    b.close()


def _oracle_follow(b, i, state, seed, nit, eta, keep):
    o = orc.MMWOracle(nit=nit, eta=eta)
    o.run(b.sizes[i]["Z"], state, lambda it, K, D: b.sketch(i, seed, it), keep_trace=keep, factor=False)
    return o


@pytest.mark.parametrize("tol,bar", [(1e-12, 1e-9), (None, 1e-5)])
def test_device_rng_follows_the_oracle(tol, bar):
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    states = sweep_states((5, 9, 15)) + [er_contention_graph(240, 0.04, 3)]
    Zs = [12, 16, 30, 14]
    nit, eta = 150, 0.04
    seeds = np.array([11, 12, 13, 14], dtype=np.uint64)
    b = _lib.BatchSolver(Zs, states, nit, eta)
    if tol is not None:
        b.set_expm(16, tol)
    def snapshot(i):
        f = {k: b.read(i, w) for k, w in (("e_this", _lib.F_E_THIS), ("e_accu", _lib.F_E_ACCU), ("Y", _lib.F_Y), ("lval", _lib.F_LVAL),
                                           ("xval", _lib.F_XVAL), ("X_half", _lib.F_XHALF))}
        f["xsum"] = b.read(i, _lib.F_XAVG) + f["xval"]  # the sums hold X_0 .. X_{i-1}; the oracle's when iteration i + 1 starts
        f["ysum"] = b.read(i, _lib.F_YAVG) + f["Y"]
        return f
    mids = {}
    for n in (1, 36, 13, 50, 50):  # 150 in calls of uneven length
        b.iterate(n, None, seeds)
        if b.iterations_done(0) == 50:
            mids = {i: snapshot(i) for i in range(len(states))}
    for i, st in enumerate(states):
        o = _oracle_follow(b, i, st, int(seeds[i]), nit, eta, keep=[49, nit - 1])
        t = o.trace
        if tol is not None:
            end = snapshot(i)
            for name in ("e_this", "e_accu", "Y", "lval", "xval", "X_half", "xsum", "ysum"):
                assert relerr(mids[i][name], t[name][0]) < bar, (i, name, "mid")
                assert relerr(end[name], t[name][1]) < bar, (i, name, "end")
        else:
            assert relerr(mids[i]["X_half"], t["X_half"][0]) < bar, i
        assert relerr(b.read(i, _lib.F_XHALF), t["X_half"][1]) < bar, i
    b.close()


def test_device_sketch_is_the_handles():
    state = sweep_states((7,))[0]
    b = _lib.BatchSolver([10], [state], 3, 0.05)
    s = _lib.Solver(10, state, 3, 0.05)
    for it in (0, 2, 17):
        assert np.array_equal(b.sketch(0, 99, it), s.sketch(99, it))
    b.iterate(2, None, [99])
    assert np.array_equal(b.read(0, _lib.F_SKETCH), s.sketch(99, 1))
    b.close()
    s.close()


FIELDS = (_lib.F_Y, _lib.F_E_ACCU, _lib.F_E_THIS, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG, _lib.F_XHALF)


def _fields(b, i):
    return [b.read(i, f) for f in FIELDS]


def test_instances_are_bitwise_independent():
    from sig_sdp_mmw_amd.graphs import er_contention_graph
    pool = sweep_states((5, 7, 9, 11, 13, 15), seeds=(0, 1, 2)) + [er_contention_graph(200, 0.05, s) for s in range(3)]
    rng = np.random.default_rng(5)
    states = [pool[k] for k in rng.integers(0, len(pool), 64)]
    Zs = [int(z) for z in rng.integers(6, 24, 64)]
    seeds = np.arange(1000, 1064, dtype=np.uint64)
    nit, eta, probe = 150, 0.04, 17
    big = _lib.BatchSolver(Zs, states, nit, eta)
    big.iterate(nit, None, seeds)
    alone = _lib.BatchSolver([Zs[probe]], [states[probe]], nit, eta)
    alone.iterate(nit, None, seeds[probe:probe + 1])
    split = _lib.BatchSolver([Zs[probe]], [states[probe]], nit, eta)
    for _ in range(30):
        split.iterate(5, None, seeds[probe:probe + 1])
    again = _lib.BatchSolver([Zs[probe]], [states[probe]], nit, eta)
    again.iterate(nit, None, seeds[probe:probe + 1])
    ref = _fields(alone, 0)
    for other, i in ((big, probe), (split, 0), (again, 0)):
        for f, a, r in zip(FIELDS, _fields(other, i), ref):
            assert np.array_equal(a, r), f
    for x in (big, alone, split, again):
        x.close()


def test_export_hands_off_to_factor_and_round():
    gs = load_golden("run_env192")
    state = state_from(gs)
    Z, eta, nit = 12, 0.05, 30
    K = state[0].shape[0]
    D = 2 * Z
    rng = np.random.default_rng(3)
    sk = np.stack([orc.sketch_rows(rng.standard_normal((K, D))) for _ in range(nit)])
    b = _lib.BatchSolver([Z], [state], nit, eta)
    b.set_expm(16, 1e-13)
    b.iterate(nit, [sk])
    h = _lib.Solver(Z, state, nit, eta, dtype=_lib.F64)
    b.export(0, h)
    assert h.iterations_done == nit
    for f in (_lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_Y, _lib.F_YAVG, _lib.F_E_ACCU):
        assert np.array_equal(h.read(f), b.read(0, f)), f
    rank = min(K - 1, (Z - 1) * 2)
    Xh = h.factor(rank, seed=1)
    o = orc.MMWOracle(nit=nit, eta=eta)
    _, Xo = o.run(Z, state, lambda i, K_, D_: sk[i], factor=True)
    assert relerr(orc.projector(Xh), orc.projector(Xo)) < 1e-6
    r = rng.standard_normal((Z, rank))
    r = r / np.linalg.norm(r, axis=1, keepdims=True)
    z, rem = h.round(Z, Xh, r)
    z_o, _, rem_o, un = orc.rounding_one_attempt(Z, Xh, state, r, randint=lambda Z_, size: np.full(size, -1))
    assert int(rem[0]) == rem_o
    assert np.array_equal(np.where(z[0] < 0, -1, z[0]), np.where(un, -1, z_o.astype(np.int64)))
    # the same sketches run on a handle itself
    s = _lib.Solver(Z, state, nit, eta, dtype=_lib.F64)
    s.set_expm(_lib.EXPM_TAYLOR, 16, 1e-13)
    s.iterate(nit, sk)
    for f in (_lib.F_LVAL, _lib.F_XAVG, _lib.F_Y, _lib.F_YAVG, _lib.F_E_ACCU):
        assert relerr(h.read(f), s.read(f)) < 1e-9, f
    Xs = s.factor(rank, seed=1)
    assert relerr(orc.projector(Xh), orc.projector(Xs)) < 1e-9
    z2, rem2 = s.round(Z, Xs, r)
    assert np.array_equal(z2, z) and np.array_equal(rem2, rem)
    # mismatches are refused
    other = _lib.Solver(Z + 1, state, nit, eta, dtype=_lib.F64)
    with pytest.raises(_lib.MMWError):
        b.export(0, other)
    f32 = _lib.Solver(Z, state, nit, eta, dtype=_lib.F32)
    with pytest.raises(_lib.MMWError):
        b.export(0, f32)
    for x in (b, h, s, other, f32):
        x.close()


def colouring_remainder(z_vec, Z, state):
    """Users whose slot breaks a constraint of the rounding (sdp_solver.py:78-92): the interference the other members of its
    slot emit onto a user exceeds its h_max, or it shares its access point with another member."""
    S = scipy.sparse.csr_matrix(state[0]).copy()
    S.setdiag(0)
    S.eliminate_zeros()
    Q = scipy.sparse.csr_matrix(state[1])
    h = np.asarray(state[2])
    z = np.asarray(z_vec).astype(np.int64)
    assert z.min() >= 0 and z.max() < Z
    same = z[:, None] == z[None, :]
    recv = np.asarray((S.multiply(same)).sum(axis=0)).ravel()  # sum over j in k's slot of S[j, k]
    clash = np.asarray((Q.multiply(same) != 0).sum(axis=1)).ravel()
    return int(np.sum((recv > h) | (clash > 0)))


def test_lockstep_search_matches_single_instance_search():
    from sig_sdp_mmw_amd import batch
    from sig_sdp_mmw_amd.binary_search import binary_search_relaxation
    states = sweep_states((5, 6, 7, 8), seeds=(0, 1, 2, 3))
    kw = dict(nit=40, eta=0.04, seed=7)
    results = batch.search_many(states, **kw)
    for i, st in enumerate(states):
        one = batch.single(st, index=i, **kw)
        bs = binary_search_relaxation()
        bs.verbose = False
        bs.feasibility_check_alg = one
        z_vec, Z_fin, rem = bs.run(st)
        assert results[i]["probes"] == one.probes, i
        assert results[i]["Z"] == Z_fin, i
        assert results[i]["remainder"] == 0 and rem == 0, i
        assert np.array_equal(results[i]["z_vec"], z_vec), i
        assert colouring_remainder(results[i]["z_vec"], results[i]["Z"], st) == 0, i
        one.close()


def test_export_before_the_last_iteration_continues_like_the_handle():
    """Export after 12 of 30 iterations: the handle's running sums, its gap and the rest of the run are those of a handle that ran
    the 12 iterations itself."""
    gs = load_golden("run_env192")
    state = state_from(gs)
    Z, eta, nit, cut = 12, 0.05, 30, 12
    K = state[0].shape[0]
    rng = np.random.default_rng(8)
    sk = np.stack([orc.sketch_rows(rng.standard_normal((K, 2 * Z))) for _ in range(nit)])
    b = _lib.BatchSolver([Z], [state], nit, eta)
    b.set_expm(16, 1e-13)
    b.iterate(cut, [sk[:cut]])
    h = _lib.Solver(Z, state, nit, eta, dtype=_lib.F64)
    h.set_expm(_lib.EXPM_TAYLOR, 16, 1e-13)
    b.export(0, h)
    s = _lib.Solver(Z, state, nit, eta, dtype=_lib.F64)
    s.set_expm(_lib.EXPM_TAYLOR, 16, 1e-13)
    s.iterate(cut, sk[:cut])
    assert h.iterations_done == cut
    for f in (_lib.F_XAVG, _lib.F_YAVG, _lib.F_LVAL, _lib.F_Y, _lib.F_E_ACCU):
        assert relerr(h.read(f), s.read(f)) < 1e-9, f
    gh, gs_ = h.gap(), s.gap()
    assert np.allclose(gh, gs_, rtol=1e-8, atol=1e-10), (gh, gs_)
    h.iterate(nit - cut, sk[cut:])
    s.iterate(nit - cut, sk[cut:])
    for f in (_lib.F_XAVG, _lib.F_YAVG, _lib.F_LVAL, _lib.F_XHALF):
        assert relerr(h.read(f), s.read(f)) < 1e-9, f
    rank = min(K - 1, (Z - 1) * 2)
    assert relerr(orc.projector(h.factor(rank, seed=1)), orc.projector(s.factor(rank, seed=1))) < 1e-8
    for x in (b, h, s):
        x.close()


def test_run_with_state_many_is_export_and_factor_per_instance():
    from sig_sdp_mmw_amd import batch
    states = sweep_states((5, 7, 9))
    Zs, nit, eta = [8, 11, 14], 40, 0.04
    seeds = np.array([21, 22, 23], dtype=np.uint64)
    out = batch.run_with_state_many(0, Zs, states, nit=nit, eta=eta, seeds=seeds)
    assert len(out) == 3
    for i, (st, Z) in enumerate(zip(states, Zs)):
        ok, Xh = out[i]
        K = st[0].shape[0]
        rank = min(K - 1, (Z - 1) * 2)
        assert ok and Xh.shape == (K, rank)
        # the same instance alone, exported by hand: bitwise the same factor
        one = _lib.BatchSolver([Z], [st], nit, eta)
        one.iterate(nit, None, seeds[i:i + 1])
        h = _lib.Solver(Z, st, nit, eta, dtype=_lib.F64)
        one.export(0, h)
        assert np.array_equal(h.factor(rank, seed=0), Xh), i
        # and a handle that ran the same device sketches itself
        s = _lib.Solver(Z, st, nit, eta, dtype=_lib.F64)
        s.set_expm(_lib.EXPM_TAYLOR, 16, 1e-9)
        s.iterate(nit, None, seed=int(seeds[i]))
        assert relerr(orc.projector(s.factor(rank, seed=0)), orc.projector(Xh)) < 1e-6, i
        for x in (one, h, s):
            x.close()


def test_refused_slot_count_leaves_the_batch_as_it_was():
    states = sweep_states((5, 7))
    Zs, nit, eta = [8, 10], 6, 0.04
    b = _lib.BatchSolver(Zs, states, nit, eta)
    b.iterate(3, None, [5, 6])
    before = [(b.read(i, _lib.F_NORM_H), _fields(b, i)) for i in range(2)]
    with pytest.raises(_lib.MMWError, match="exceeds the batch limit"):
        b.set_slots([9, 300], nit)  # the second instance's D = 600 is over the limit; the first had been rebound already
    b._load_sizes()
    assert [b.sizes[i]["Z"] for i in range(2)] == Zs and [b.iterations_done(i) for i in range(2)] == [3, 3]
    for i in range(2):
        assert np.array_equal(b.read(i, _lib.F_NORM_H), before[i][0])
        for f, a, r in zip(FIELDS, _fields(b, i), before[i][1]):
            assert np.array_equal(a, r), (i, f)
    # and it continues exactly like a batch that was never asked
    b.iterate(3, None, [5, 6])
    ref = _lib.BatchSolver(Zs, states, nit, eta)
    ref.iterate(6, None, [5, 6])
    for i in range(2):
        for f, a, r in zip(FIELDS, _fields(b, i), _fields(ref, i)):
            assert np.array_equal(a, r), (i, f)
    b.close()
    ref.close()
