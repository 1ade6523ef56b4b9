"""Host side of the batch's warm-started probes (no GPU): the entry is declared and exported, a host-only batch refuses it, the
search rejects a bad warm_fraction before it touches a device, and the CPU restatement the GPU tests are held to
(tests/helpers/warm_oracle.py) is itself checked against `MMWOracle.run`."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, state_from
from oracle import mmw_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import warm_oracle  # noqa: E402

from sig_sdp_mmw_amd import _lib, batch  # noqa: E402


def test_warm_entry_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mmw_hip.h")).read()
    assert "int mmw_batch_set_slots_warm(mmw_batch* b, const int32_t* Z, int32_t nit);" in hdr
    assert "mmw_batch_set_slots_warm" in _lib.EXPORTS
    getattr(_lib.lib(), "mmw_batch_set_slots_warm")


def test_host_only_batch_refuses_a_warm_slot_change():
    g = load_golden("run_dense60")
    b = _lib.BatchSolver([int(g["Z"])], [state_from(g)], 3, 0.05, device=-1)
    with pytest.raises(_lib.MMWError, match="device -1"):
        b.set_slots([4], 3, warm=True)
    b.close()


@pytest.mark.parametrize("bad", [0.0, -0.5, 1.5, float("nan")])
def test_search_rejects_a_warm_fraction_outside_0_1(bad):
    g = load_golden("run_dense60")
    with pytest.raises(ValueError, match="warm_fraction"):
        batch.search_many([state_from(g)], nit=3, warm_start=True, warm_fraction=bad, device=-1)
    with pytest.raises(ValueError, match="warm_fraction"):
        batch.single(state_from(g), warm_start=True, warm_fraction=bad, device=-1)


def test_warm_iterations_is_the_rule_of_the_mmw_class():
    assert [batch.warm_iterations(n, 1.0 / 3.0) for n in (1, 2, 3, 60, 150, 151)] == [1, 1, 1, 20, 50, 51]
    assert batch.warm_iterations(150, 1.0) == 150 and batch.warm_iterations(150, 1e-9) == 1


@pytest.mark.parametrize("name", ["env75", "dense60"])
def test_warm_oracle_with_kept_sums_is_one_run(name):
    g = load_golden("run_" + name)
    state, Z, eta = state_from(g), int(g["Z"]), float(g["eta"])
    n1, n2 = 3, 2
    sk = g["randv"][:n1 + n2]
    o = orc.MMWOracle(nit=n1 + n2, eta=eta)
    o.run(Z, state, lambda i, K, D: sk[i], keep_trace=[n1 + n2 - 1], factor=False)
    w = warm_oracle.run(Z, n1, Z, n2, state, eta, lambda i, K, D: sk[i], lambda i, K, D: sk[n1 + i], keep_sums=True)
    t = o.trace
    for key in ("lval", "xval", "Y", "e_accu", "e_this", "X_half"):
        assert np.array_equal(w[key], t[key][0]), key
    assert np.allclose(w["xsum"], o.xavg * (n1 + n2), rtol=0, atol=1e-14)  # (the oracle keeps the sum divided by nit)
    assert np.array_equal(w["xsum"] + w["xval"], t["xsum"][0]) and np.array_equal(w["ysum"] + w["Y"], t["ysum"][0])
    # and with the sums restarted, they hold the kept X / Y and n2 - 1 new terms: what is left of the whole run's after the first n1
    r = warm_oracle.run(Z, n1, Z, n2, state, eta, lambda i, K, D: sk[i], lambda i, K, D: sk[n1 + i])
    first = orc.MMWOracle(nit=n1, eta=eta)
    first.run(Z, state, lambda i, K, D: sk[i], factor=False)
    assert np.allclose(r["xsum"], w["xsum"] - first.xavg * n1, rtol=0, atol=1e-13)
    assert abs(r["ysum"].sum() - n2) < 1e-12
    assert np.array_equal(r["xval"], w["xval"]) and np.array_equal(r["lval"], w["lval"])
