"""The generator as DESIGN.md section 2 defines it, on the CPU: tests/helpers/philox_ref.py against Random123's published Philox4x32-10
vectors, the sketch it defines against what the algorithm needs of it (uniform unit rows, independent across rows and iterations),
the separation of its streams, and the formulas at the extreme words.  test_hip_sketch_rng.py then holds the kernels to this
reference; nothing here touches the library.

The statistical conditions are on FIXED inputs (K = 4096, D = 64, iteration 0, three seeds, both Box-Muller forms), not
measurements: with these inputs the reference gives KS p-values 0.22 ... 0.94, sqrt(K) max |off-diagonal| 3.1 ... 3.8,
sqrt(K) max |diagonal - 1| 3.1 ... 4.4 and normalised cross-iteration inner products 0.6 ... 1.8 (a |N(0, 1)| each).  An input
changed is a condition to re-check.
"""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.stats

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import philox_ref as pr  # noqa: E402

KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, out):
    got = pr.philox4x32_10(*ctr, *key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(x) for x in got] == list(out), [hex(int(x)) for x in got]


def test_philox_is_vectorised_over_every_counter_word():
    """A grid of counters in one call is the calls one by one (the sketch draws rows x groups at once)."""
    r, p = np.arange(3)[:, None], np.arange(5)[None, :]
    got = pr.philox4x32_10(r, p, 7, pr.TAG_SKETCH, 11, 13)
    assert got.shape == (3, 5, 4)
    for i in range(3):
        for j in range(5):
            assert np.array_equal(got[i, j], pr.philox4x32_10(i, j, 7, pr.TAG_SKETCH, 11, 13))
    assert np.array_equal(pr.philox4x32_10(*(np.full(2, 0xffffffff),) * 4, 0xffffffff, 0xffffffff)[1], np.array(KAT[1][2], dtype=np.uint32))


# ---- the generator as defined is a good sketch ------------------------------------------------------------------------------------
K_STAT, D_STAT = 4096, 64
SEEDS = [1, 12345, (7 << 32) | 1]
FORMS = ["f64", "f32"]


@functools.lru_cache(maxsize=None)
def block(seed, iteration, form):
    b = pr.sketch(K_STAT, D_STAT, seed, iteration, form)
    b.setflags(write=False)
    return b


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_rows_are_uniform_on_the_sphere(seed, form):
    """A coordinate of a uniform unit vector of R^D has its square distributed Beta(1/2, (D - 1)/2), exactly; the second moment
    (D/K) R^T R is the identity to the sampling error 1/sqrt(K) of K independent rows."""
    R = block(seed, 0, form)
    assert np.all(np.isfinite(R))
    assert np.max(np.abs(np.linalg.norm(R, axis=1) - 1.0)) <= 4 * np.finfo(np.float64).eps
    p = scipy.stats.kstest((R * R).ravel(), scipy.stats.beta(0.5, (D_STAT - 1) / 2.0).cdf).pvalue
    G = (D_STAT / K_STAT) * (R.T @ R)
    off = np.sqrt(K_STAT) * np.max(np.abs(G - np.diag(np.diag(G))))
    dia = np.sqrt(K_STAT) * np.max(np.abs(np.diag(G) - 1.0))
    print("sketch stats seed %d %s: KS p %.3f, sqrt(K) max off-diagonal %.2f, sqrt(K) max |diagonal - 1| %.2f" % (seed, form, p, off, dia))
    assert p > 1e-3
    assert off < 6.0
    assert dia < 7.0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_iterations_draw_independent_blocks(seed, form):
    """<R0, R1> of two independent blocks is a sum of K D products of variance 1/D^2: |<R0, R1>| D / sqrt(K D) is a |N(0, 1)|."""
    t = abs(float(np.sum(block(seed, 0, form) * block(seed, 1, form)))) * D_STAT / np.sqrt(K_STAT * D_STAT)
    print("sketch stats seed %d %s: normalised <R0, R1> %.3f" % (seed, form, t))
    assert t < 5.0


# ---- separation ---------------------------------------------------------------------------------------------------------------
def far_apart(a, b):
    """Two blocks of unit rows that share nothing: independent rows have |<a_i, b_i>| ~ 1/sqrt(D); a shared word would show as a
    coordinate pair that agrees."""
    return not np.any(a == b) and np.max(np.abs(a - b)) > 0.1


@pytest.mark.parametrize("form", FORMS)
def test_the_high_word_of_the_seed_is_part_of_the_key(form):
    a, b, c = (pr.sketch(70, 9, s, 3, form) for s in (5, (1 << 32) | 5, (1 << 63) | 5))
    assert far_apart(a, b) and far_apart(a, c) and far_apart(b, c)
    assert far_apart(pr.sketch(70, 9, 1 << 32, 3, form), pr.sketch(70, 9, 0, 3, form))
    assert far_apart(pr.sketch(70, 9, 1, 3, form), pr.sketch(70, 9, 1 << 32, 3, form))  # the two key words are not interchangeable


def test_sketch_and_randv_of_the_same_seed_and_index_differ():
    for seed, i in ((0, 0), (12345, 7)):
        assert far_apart(pr.sketch(70, 9, seed, i, "f64"), pr.randv(70, 9, seed, i))


@pytest.mark.parametrize("form", FORMS)
def test_row_and_iteration_are_different_counter_words(form):
    """Row r of iteration i is not row i of iteration r; nor is (row, group) symmetric."""
    n = 6
    blocks = np.stack([pr.sketch(n, 8, 9, i, form) for i in range(n)])  # [iteration, row, column]
    assert far_apart(blocks[np.triu_indices(n, 1)], np.swapaxes(blocks, 0, 1)[np.triu_indices(n, 1)])
    per = 2 if form == "f64" else 4
    w = pr.sketch(n, n * per, 9, 0, form).reshape(n, n, per)  # [row, group, within]
    assert far_apart(w[np.triu_indices(n, 1)], np.swapaxes(w, 0, 1)[np.triu_indices(n, 1)])


@pytest.mark.parametrize("form", FORMS + ["randv"])
@pytest.mark.parametrize("D", [1, 3, 5, 7, 129, 257])
def test_odd_widths_have_unit_rows_and_are_a_prefix_of_the_draw(D, form):
    """Columns >= D do not count: the norm is over D columns (D = 1 leaves +-1), and before normalisation a narrower row is the
    prefix of a wider one."""
    draw = (lambda d: pr.randv(40, d, 3, 2)) if form == "randv" else (lambda d: pr.sketch(40, d, 3, 2, form))
    R = draw(D)
    assert R.shape == (40, D) and np.all(np.isfinite(R))
    assert np.max(np.abs(np.linalg.norm(R, axis=1) - 1.0)) <= 4 * np.finfo(np.float64).eps
    if D == 1:
        assert np.all(np.abs(R) == 1.0) and np.any(R > 0) and np.any(R < 0)
    wide = draw(D + 3)[:, :D]
    assert np.max(np.abs(R - wide / np.linalg.norm(wide, axis=1)[:, None])) <= 4 * np.finfo(np.float64).eps


# ---- extreme words (the formulas only) --------------------------------------------------------------------------------------------
ONES = np.full(4, 0xffffffff, dtype=np.uint32)
ZEROS = np.zeros(4, dtype=np.uint32)


def test_all_ones_words_give_zero_radius():
    """u1 = 1 exactly in every form: r = 0 and both normals of a radius are exactly 0, not NaN."""
    for n in (pr.normals_f64(ONES), pr.normals_f32(ONES, np.float64), pr.normals_f32(ONES, np.float32)):
        assert np.all(n == 0.0), n


def test_all_zero_words_give_the_largest_finite_normals():
    """u1 at its smallest, 2^-53 or 2^-24: r = sqrt(106 ln 2) = 8.572 or sqrt(48 ln 2) = 5.768, angle 0."""
    n64 = pr.normals_f64(ZEROS)
    assert np.all(np.isfinite(n64)) and np.max(np.abs(n64)) <= 8.6
    assert n64[0] == pytest.approx(np.sqrt(106 * np.log(2.0)), rel=1e-15) and n64[1] == 0.0
    for ft in (np.float64, np.float32):
        n32 = pr.normals_f32(ZEROS, ft)
        assert n32.dtype == ft and np.all(np.isfinite(n32)) and np.max(np.abs(n32)) <= 5.77
        assert n32[0] == pytest.approx(np.sqrt(48 * np.log(2.0)), rel=1e-6) and n32[1] == 0.0 and n32[3] == 0.0


def test_no_nan_or_inf_anywhere_on_the_word_edges():
    """Every combination of the words {0, 1, 2^8 - 1, 2^8, 2^11 - 1, 2^11, 2^31, 2^32 - 2^8, 2^32 - 1}: the edges of the shifts."""
    e = np.array([0, 1, 255, 256, 2047, 2048, 1 << 31, (1 << 32) - 256, (1 << 32) - 1], dtype=np.uint32)
    w = np.stack(np.meshgrid(e, e, e, e, indexing="ij"), axis=-1).reshape(-1, 4)
    n64 = pr.normals_f64(w)
    assert np.all(np.isfinite(n64)) and np.max(np.abs(n64)) <= 8.6
    for ft in (np.float64, np.float32):
        n32 = pr.normals_f32(w, ft)
        assert np.all(np.isfinite(n32)) and np.max(np.abs(n32)) <= 5.77


def test_the_fp32_yardstick_is_what_the_contract_records():
    """e_ref = max |sketch in float32 - sketch in float64| on the same words, about 1.5e-6 / sqrt(D): the figures DESIGN.md states."""
    for D, lo, hi in ((4, 1e-7, 1e-6), (64, 5e-8, 5e-7), (1024, 1e-8, 1.5e-7)):
        e = pr.sketch_f32_yardstick(70, D, 1, 0)
        print("fp32 yardstick D %d: e_ref %.2e" % (D, e))
        assert lo < e < hi, (D, e)
