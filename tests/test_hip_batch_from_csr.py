"""A batch built on the device from CSR states that lie there (mmw_batch_create_from_csr, csrc/kernels_batch_csr_pattern.h,
csrc/batch_from_csr.h) against the batch mmw_batch_create makes from the host copies of the same states: every list equal, every fp64
field equal on its raw bits, the sizes equal; everything downstream bitwise the same; an instance the same alone and among neighbours;
the batch keeps nothing of the states it was built from; the refusals; and the workflows routed through it.

The cases are tests/helpers/csr_cases.py's (the smallest shapes at which the kernels can go wrong: K = 2, null Q pointers, the 64-wide
trips one over full, stored zeros, missing diagonals, the golden states, K = 768 with more rows than threads) and `valid6`, which has
gains on association pairs and a user that neither emits nor hears."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse

from conftest import ROOT
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import csr_cases as cc  # noqa: E402
from sig_sdp_mmw_amd import _lib, batch  # noqa: E402
from test_hip_batch_shapes import FIELDS  # noqa: E402

pytestmark = pytest.mark.gpu

ETA = 0.04
NIT = 3
NAMES = list(cc.CASES) + ["valid6"]
I_LISTS = tuple(getattr(_lib, f) for f in cc.I_FIELDS)
I_LAZY = tuple(f for f in I_LISTS if f != _lib.I_L_INDPTR)
F_EAGER = (_lib.F_S_SUM, _lib.F_NORM_H, _lib.BATCH_F_PATTERN) + FIELDS  # what never needs a host list


@functools.lru_cache(maxsize=None)
def case(name):
    """(state, Z): shared and left unchanged."""
    if name == "valid6":
        sp, si, sx, qp, qi, qx, h = cc.valid6()
        return (scipy.sparse.csr_matrix((sx, si, sp), shape=(6, 6)), scipy.sparse.csr_matrix((qx, qi, qp), shape=(6, 6)), h), 3
    return cc.case(name)


def zs(names):
    return [case(n)[1] for n in names]


def upload(names):
    return [_lib.DeviceCSR.upload(case(n)[0]) for n in names]


def close(*hs):
    for h in hs:
        h.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64)


def same_f64(x, y, inst_x, inst_y, fields, what):
    for f in fields:
        a, b = x.read(inst_x, f), y.read(inst_y, f)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, "f64 field", f)


def same_i32(x, y, inst_x, inst_y, fields, what):
    for f in fields:
        assert np.array_equal(x.read_i32(inst_x, f), y.read_i32(inst_y, f)), (what, "i32 field", f)


def same_instance(x, y, i, j, what):
    assert x.sizes[i] == y.sizes[j], what
    same_f64(x, y, i, j, F_EAGER + (_lib.F_ST_DATA,), what)
    same_i32(x, y, i, j, I_LISTS + (_lib.I_PATTERN,), what)


def build_info(b, inst):
    return [int(v) for v in b.read(inst, _lib.BATCH_F_BUILD_INFO)]


def snapshot(b, inst):
    """Everything of an instance that needs no host list, as raw bits."""
    return ([bits(b.read(inst, f)).copy() for f in F_EAGER], b.read_i32(inst, _lib.I_PATTERN).copy(), b.read_i32(inst, _lib.I_L_INDPTR).copy(),
            dict(b.sizes[inst]))


def same_snapshot(s, t):
    return all(np.array_equal(a, b) for a, b in zip(s[0], t[0])) and np.array_equal(s[1], t[1]) and np.array_equal(s[2], t[2]) and s[3] == t[3]


class Pair:
    """Every case in one batch built on the device from uploaded states, and the batch built on the host from the host triples; shared
    by the tests below, which read and do not iterate."""

    def __init__(self):
        self.csrs = upload(NAMES)
        self.dev = _lib.BatchSolver.from_csr(self.csrs, zs(NAMES), NIT, ETA)
        self.host = _lib.BatchSolver(zs(NAMES), [case(n)[0] for n in NAMES], NIT, ETA)


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    close(p.dev, p.host, *p.csrs)


def test_every_field_of_every_case_is_the_host_builds(pair):
    dev, host = pair.dev, pair.host
    assert (dev.B, dev.nits, dev.active, dev.device) == (host.B, host.nits, host.active, host.device)
    assert dev.sizes == host.sizes
    for i, n in enumerate(NAMES):
        for k, v in cc.EXPECTED_SIZES.get(n, {}).items():
            assert dev.sizes[i][k] == v, (n, k)
        assert build_info(host, i) == [0, 1]
        assert build_info(dev, i) == [1, 0]
        same_f64(dev, host, i, i, F_EAGER, n)
        same_i32(dev, host, i, i, (_lib.I_PATTERN, _lib.I_L_INDPTR), n)
        assert build_info(dev, i) == [1, 0], "a field that needs no host list completed them"
        same_i32(dev, host, i, i, I_LISTS, n)
        same_f64(dev, host, i, i, (_lib.F_ST_DATA,), n)
        assert build_info(dev, i) == [1, 1]
        same_f64(dev, host, i, i, F_EAGER, n)  # completing the lists changed no value


def test_downstream_is_bitwise_the_host_built_batchs():
    B = len(NAMES)
    Z = zs(NAMES)
    seeds = np.arange(21, 21 + B, dtype=np.uint64)
    csrs = upload(NAMES)
    states = [case(n)[0] for n in NAMES]
    dev = _lib.BatchSolver.from_csr(csrs, Z, NIT, ETA)
    host = _lib.BatchSolver(Z, states, NIT, ETA)
    close(*csrs)
    for b in (dev, host):
        b.iterate(NIT, None, seeds)
    for i, n in enumerate(NAMES):
        same_f64(dev, host, i, i, FIELDS + (_lib.F_SKETCH,), n)
    for b in (dev, host):
        b.set_slots([z - 1 for z in Z], NIT)
    assert dev.sizes == host.sizes
    for i, n in enumerate(NAMES):
        same_f64(dev, host, i, i, F_EAGER, n)
    take = [dev.sizes[i]["K"] <= _lib.BATCH_EPILOGUE_MAX_K for i in range(B)]
    assert [n for n, t in zip(NAMES, take) if not t] == ["journal16"]  # (K = 2048: it iterates in the batch and takes no epilogue there)
    for b in (dev, host):
        b.iterate(NIT, None, seeds)
        b.factor(take)
    rd, rh = dev.round(4, seeds, take), host.round(4, seeds, take)
    for i, n in enumerate(NAMES):
        same_f64(dev, host, i, i, FIELDS, n)
        if take[i]:
            assert np.array_equal(bits(dev.read_factor(i)), bits(host.read_factor(i))), n
        assert build_info(dev, i) == [1, 0], "iterating, a slot change, factoring and rounding need no host list"
    for i in range(B):
        if take[i]:
            assert all(np.array_equal(a[i], b[i]) for a, b in zip(rd, rh)), NAMES[i]
        else:
            assert rd[0][i] is None and rh[0][i] is None
    # the greedy baseline on the generator-made case it takes (it refuses a Q that is no union of cliques, which rules out the ER
    # cases, and K over the epilogue's limit, which rules out journal16 on either batch): the clique decision of EVERY instance comes
    # from the batch's own copy of Q and completes no host list
    who = [NAMES.index("golden_env75")]
    tk = [i in who for i in range(B)]
    Zm = [z - 1 for z in Z]
    gd, gh = dev.gm(0, Zm, take=tk, keys=True), host.gm(0, Zm, take=tk, keys=True)
    for i in who:
        assert np.array_equal(gd[0][i], gh[0][i]) and np.array_equal(bits(gd[3][i]), bits(gh[3][i]))
    assert np.array_equal(np.asarray(gd[1])[tk], np.asarray(gh[1])[tk]) and np.array_equal(np.asarray(gd[2])[tk], np.asarray(gh[2])[tk])
    said = []
    for b in (dev, host):
        with pytest.raises(_lib.MMWError) as ei:
            b.gm(0, Zm, take=[n == "journal16" for n in NAMES])
        said.append(str(ei.value))
    assert said[0] == said[1] and "instance %d: K = 2048 exceeds the limit" % NAMES.index("journal16") in said[0]
    assert all(build_info(dev, i) == [1, 0] for i in range(B))
    # export into a handle
    for n in ("k3", "er120_holes", "golden_env75"):
        i = NAMES.index(n)
        s1, s2 = (_lib.Solver(Z[i] - 1, states[i], NIT, ETA) for _ in range(2))
        dev.export(i, s1)
        host.export(i, s2)
        for f in (_lib.F_Y, _lib.F_E_ACCU, _lib.F_LVAL, _lib.F_XVAL, _lib.F_XAVG, _lib.F_YAVG):
            assert np.array_equal(bits(s1.read(f)), bits(s2.read(f))), (n, f)
        assert s1.iterations_done == s2.iterations_done == NIT
        close(s1, s2)
    close(dev, host)


@pytest.mark.parametrize("name", ["k2", "er65", "journal16"])
def test_alone_and_among_neighbours(pair, name):
    k = NAMES.index(name)
    c = _lib.DeviceCSR.upload(case(name)[0])
    one = _lib.BatchSolver.from_csr([c], [case(name)[1]], NIT, ETA)
    c.close()
    assert same_snapshot(snapshot(one, 0), snapshot(pair.dev, k))
    same_instance(one, pair.dev, 0, k, name)
    one.close()


def test_the_same_state_twice_gives_two_equal_instances(pair):
    k = NAMES.index("er120_zeros")
    c = pair.csrs[k]
    two = _lib.BatchSolver.from_csr([c, c.device_state()], [6, 6], NIT, ETA)
    same_instance(two, two, 0, 1, "twice")
    same_instance(two, pair.dev, 1, k, "twice against the full batch")
    two.close()


def test_the_batch_keeps_nothing_of_the_states(pair):
    names = ["k3", "er130", "golden_dense60", "valid6"]
    idx = [NAMES.index(n) for n in names]
    seeds = np.arange(5, 5 + len(names), dtype=np.uint64)
    csrs = upload(names)
    dev = _lib.BatchSolver.from_csr(csrs, zs(names), NIT, ETA)
    close(*csrs)
    filler = upload(names)  # (whatever the allocator hands out next may be the memory just freed)
    host = _lib.BatchSolver(zs(names), [case(n)[0] for n in names], NIT, ETA)
    for i, n in enumerate(names):
        assert build_info(dev, i) == [1, 0]
        same_i32(dev, pair.host, i, idx[i], I_LAZY, n)
        same_f64(dev, pair.host, i, idx[i], (_lib.F_ST_DATA,), n)
        assert build_info(dev, i) == [1, 1]
    for b in (dev, host):
        b.iterate(NIT, None, seeds)
        b.factor()
    rd, rh = dev.round(4, seeds), host.round(4, seeds)
    for i, n in enumerate(names):
        same_f64(dev, host, i, i, FIELDS, n)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for x, y in zip(rd, rh) for a, b in zip(x, y))
    close(dev, host, *filler)


def test_borrowed_pointers(pair):
    """wrap on the addresses of uploaded states (k3: the Q pointers are null): the same instances."""
    names = ["k3", "er120", "journal16"]
    ws = []
    for n in names:
        up = pair.csrs[NAMES.index(n)]
        ptr = up.pointers()
        if n == "k3":
            assert ptr[4] == 0 and ptr[5] == 0
        ws.append(_lib.DeviceCSR.wrap(*ptr, K=up.K, nnzS=up.nnzS, nnzQ=up.nnzQ))
    b = _lib.BatchSolver.from_csr(ws, zs(names), NIT, ETA)
    close(*ws)
    for i, n in enumerate(names):
        same_instance(b, pair.dev, i, NAMES.index(n), n)
    b.close()


def test_states_borrowed_from_torch_and_freed():
    """er120 and golden_env75 as torch sparse-CSR tensors, borrowed by DeviceCSR.from_torch, built into a batch, then closed and the
    tensors deleted before the batch completes its lists and iterates.  torch has to touch the device before the library's first HIP
    call in a process, so the case runs in a fresh interpreter: tests/helpers/batch_csr_torch_child.py."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "batch_csr_torch_child.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "batch from_torch ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("kind", cc.DEVICE_SAFE)
def test_malformed_instance_is_refused_on_the_device(pair, kind):
    """Only the kinds whose bad value is never used as an address.  The refusal leaves nothing behind: a valid batch made afterwards is the
    one made before."""
    K, Z, arrays = cc.malformed(kind)
    k = NAMES.index("valid6")
    good = pair.csrs[k]
    bad = _lib.DeviceCSR.upload_arrays(K, arrays)
    with pytest.raises(_lib.MMWError) as ei:
        _lib.BatchSolver.from_csr([good, bad, good], [3, Z, 3], NIT, ETA)
    assert "status -1: mmw_batch_create_from_csr: instance 1: " + cc.MALFORMED[kind] in str(ei.value), str(ei.value)
    after = _lib.BatchSolver.from_csr([good, pair.csrs[NAMES.index("er65")]], [3, 8], NIT, ETA)
    same_instance(after, pair.dev, 0, k, "after a refusal")
    same_instance(after, pair.dev, 1, NAMES.index("er65"), "after a refusal")
    close(after, bad)


def test_other_refusals_on_the_device(pair):
    good = pair.csrs[NAMES.index("valid6")]
    host_only = _lib.DeviceCSR.upload_arrays(6, cc.valid6(), device=-1)
    for mix in ([good, host_only], [host_only, good]):  # (instance 0 is what every other one is held against)
        with pytest.raises(_lib.MMWError, match=r"status -1: mmw_batch_create_from_csr: instance 1: host-only states \(device -1\) and states on a device"):
            _lib.BatchSolver.from_csr(mix, [3, 3], NIT, ETA)
    K, Z, arrays = cc.malformed("zero_norm_H")
    zero = _lib.DeviceCSR.upload_arrays(K, arrays)
    with pytest.raises(_lib.MMWError, match=r"status -1: mmw_batch_create_from_csr: instance 2: norm_H has a zero entry"):
        _lib.BatchSolver.from_csr([good, good, zero], [3, 3, Z], NIT, ETA)
    with pytest.raises(_lib.MMWError, match=r"status -1: mmw_batch: instance 1: D = 600 exceeds the batch limit 512 \(run it on a handle\)"):
        _lib.BatchSolver.from_csr([good, good], [3, 300], NIT, ETA)
    after = _lib.BatchSolver.from_csr([good], [3], NIT, ETA)
    same_instance(after, pair.dev, 0, NAMES.index("valid6"), "after the refusals")
    close(after, host_only, zero)


# ---- the workflows ------------------------------------------------------------------------------------------------------------------
WF = ["er120_holes", "er120", "golden_env75", "valid6"]


def wf_states():
    csrs = upload(WF)
    return csrs, [c.device_state() for c in csrs], [c.state() for c in csrs]


def same_result(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_search_many_in_the_batch_is_the_host_routes():
    csrs, dev_states, triples = wf_states()
    got = batch.search_many(dev_states, nit=12, eta=ETA, seed=3, nattempt=4, epilogue="batch")
    want = batch.search_many(triples, nit=12, eta=ETA, seed=3, nattempt=4, epilogue="batch")
    assert len(got) == len(want) == len(WF)
    for g, w in zip(got, want):
        same_result(g, w)
    assert all(s._host is None for s in dev_states)
    close(*csrs)


def test_run_with_state_many_and_convergence_many_are_the_host_routes():
    csrs, dev_states, triples = wf_states()
    Z = zs(WF)
    got = batch.run_with_state_many(0, Z, dev_states, nit=8, eta=ETA, epilogue="batch")
    want = batch.run_with_state_many(0, Z, triples, nit=8, eta=ETA, epilogue="batch")
    for (ok1, x1), (ok2, x2) in zip(got, want):
        assert ok1 and ok2 and x1.shape == x2.shape and np.array_equal(bits(x1), bits(x2))
    got = batch.convergence_many(Z, dev_states, 6, ETA)
    want = batch.convergence_many(Z, triples, 6, ETA)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g["gap"]), bits(w["gap"])) and np.array_equal(g["lanczos_steps"], w["lanczos_steps"])
    assert all(s._host is None for s in dev_states)
    close(*csrs)


def test_search_many_with_handles_is_the_host_routes():
    names = ["er120", "valid6"]
    csrs = upload(names)
    dev_states = [c.device_state() for c in csrs]
    got = batch.search_many(dev_states, nit=12, eta=ETA, seed=3, nattempt=4, epilogue="handle")
    want = batch.search_many([c.state() for c in csrs], nit=12, eta=ETA, seed=3, nattempt=4, epilogue="handle")
    for g, w in zip(got, want):
        assert g["Z"] == w["Z"] and g["probes"] == w["probes"] and np.array_equal(g["z_vec"], w["z_vec"])
    assert all(s._host is None for s in dev_states)
    close(*csrs)
