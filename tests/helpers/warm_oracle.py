"""CPU restatement of a warm-started probe, composed from the public pieces of oracle.mmw_oracle -- TEST INFRASTRUCTURE.

Two probes on one state: n1 iterations at Z1 as `MMWOracle.run` runs them (mmw.py:75-200), then the slot count changes to Z2 and
n2 more iterations continue from the iterate the first probe left.  The pattern of L / X does not depend on Z; the Z-dependent
scalars (norm_H, cH and the coefficients of the violations and of the loss) are those of `Pattern(Z2, state)`.  What is kept across
the change is (e_accu, lval, xval, Y); the running sums restart at zero (`keep_sums=True` keeps them instead: with Z2 = Z1 the two
probes are then one run of n1 + n2 iterations, which is how tests/test_batch_warm_host.py checks this helper).

The sums follow the oracle's (and the batch's) convention: iteration i adds X_i and Y_i when it starts.  After the n2 warm
iterations `xsum` / `ysum` therefore hold the kept X / Y and n2 - 1 new terms.  A handle restarts its sums from the kept X / Y and adds every new X_i / Y_i as
soon as it is made while iterations remain, so after all n2 announced iterations it holds the same n2 terms.
"""
import numpy as np

from oracle import mmw_oracle as orc


def _iterate(p, st, eta, sketch, it0, n, D, expm):
    for i in range(n):
        st["xsum"] = st["xsum"] + st["xval"]
        st["ysum"] = st["ysum"] + st["Y"]
        e_this = orc.violations(p, st["xval"])
        st["e_accu"] = st["e_accu"] + e_this * eta
        st["Y"] = orc.softmax(st["e_accu"])
        st["lval"] = st["lval"] - orc.loss_values(p, st["Y"]) * eta
        X_half = expm(p.csr(st["lval"] / 2.0), sketch(it0 + i, p.K, D))
        st["xval"] = orc.x_on_pattern(p, X_half)
        st["e_this"], st["X_half"] = e_this, X_half
    return st


def run(Z1, n1, Z2, n2, state, eta, sketch1, sketch2, rank_radio=2, keep_sums=False, expm=orc.expm_half):
    """sketch1(i, K, D1) / sketch2(i, K, D2): the row-normalised sketch of iteration i of the first / second probe (the second
    probe counts from 0 again, as the solver's iteration counter does).  Returns the final iterate and the sums as a dict:
    lval, xval, Y, e_accu, e_this, X_half, xsum, ysum, and the pattern of the second probe as "pattern"."""
    p1 = orc.Pattern(Z1, state)
    C = p1.C
    xval = np.zeros(p1.nnzL)
    xval[p1.diag_pos] = 1.0
    st = {"Y": np.ones(C) / C, "e_accu": np.zeros(C), "lval": np.zeros(p1.nnzL), "xval": xval, "xsum": np.zeros(p1.nnzL), "ysum": np.zeros(C)}
    st = _iterate(p1, st, eta, sketch1, 0, n1, Z1 * rank_radio, expm)
    p2 = orc.Pattern(Z2, state)
    assert np.array_equal(p1.row, p2.row) and np.array_equal(p1.col, p2.col), "the pattern does not depend on Z"
    if not keep_sums:
        st["xsum"] = np.zeros(p2.nnzL)
        st["ysum"] = np.zeros(C)
    st = _iterate(p2, st, eta, sketch2, 0, n2, Z2 * rank_radio, expm)
    st["pattern"] = p2
    return st
