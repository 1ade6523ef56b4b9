"""MAX_RAND's device draw restated in NumPy from its statement in include/mmw_hip.h (mmw_gm_rand), and the cases its tests share.

The words come from `philox_ref.philox4x32_10` (held to Random123's vectors by test_sketch_rng_host.py) with the counter (row, column
pair, attempt, TAG) under the key (seed low word, seed high word); the two uniforms are `philox_ref.normals_f64`'s.  The header
states that ln, cos and sin are one fixed sequence of IEEE double operations rather than a math library's functions, so that a
host-only handle and the device agree bit for bit; `normals` below follows that sequence in NumPy's float64 arithmetic (every +, *,
/ and sqrt of NumPy is the IEEE operation, none is fused) and `test_gm_rand_host.py` holds it to `math.log` / `math.cos` / `math.sin`
within a few ulp, so the restatement is checked against the definition it claims to evaluate.

    normals(words)                          -> float64 [..., 2]
    draw(K, Z, seed, attempt)               -> (pref_val float64 [K, Z], order_key float64 [K])
    tables(pref_val, order_key)             -> (rank int64 [K], pref int64 [K, Z])   the order and the preference rows
    reference(Z, state, seed, nattempt)     -> (slots int64 [nattempt, K] with -1, rem list)   gm_restate.max_rand on those tables
    pick_of(rem, rule)                      -> the attempt the two rules choose
    state(name)                             -> the states the tests share, built once by the project's generators
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gm_restate  # noqa: E402
import philox_ref as pr  # noqa: E402

TAG_PREF = 0x47525046  # "GRPF"
TAG_KEY = 0x47524B59   # "GRKY"

LG = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
      1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)
LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
     -2.50507602534068634195e-08, 1.58969099521155010221e-10)
CC = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
      2.08757232129817482790e-09, -1.13596475577881948265e-11)


RHO = 75e-4  # three stations per cell, the journal sweeps' density
DRAW_SHAPES = ((2, 1), (2, 2), (64, 63), (65, 64), (65, 65), (192, 7))  # (K, Z): odd and even Z, a wave and one more, several blocks
DRAW_SEEDS = (5, (0x9E3779B9 << 32) | 0x7F4A7C15)  # the second checks the key's upper word
DRAW_ATTEMPTS = (0, 3)
STATE_OF_K = {2: "one_ap", 64: "er64", 65: "er65", 192: "j8", 675: "j15", 1024: "k1024"}
_states = {}


def state(name):
    """The states the tests share, each built once by the project's own generators (or read from tests/golden) and left unchanged."""
    if name not in _states:
        from conftest import load_golden, state_from
        from sig_sdp_mmw_amd.graphs import _state_at, er_contention_graph, journal_graph
        if name == "one_ap":  # K = 2 behind one access point: Q is the 2-clique
            st = _state_at(np.array([[3.0, 4.0], [15.5, 12.25]]), np.array([[10.0, 10.0]]))[0]
        elif name == "er64":
            st = er_contention_graph(64, 0.15, seed=2)
        elif name == "er65":
            st = er_contention_graph(65, 0.15, seed=3)
        elif name == "er1025":  # one user over the batch's limit
            st = er_contention_graph(1025, 0.004, seed=4)
        elif name == "k1024":  # 16 x 16 cells with four stations each: the batch's limit exactly
            st = journal_graph(16, 0.01, seed=1)
        elif name in ("env75", "env300", "er120"):
            st = state_from(load_golden("run_" + name))
        elif name.startswith("j"):
            st = journal_graph(int(name[1:]), RHO, seed=int(name[1:]) % 4)
        else:
            raise KeyError(name)
        _states[name] = st
    return _states[name]


def uniforms(words):
    """(u1 in (0, 1], u2 in [0, 1)) of four words, as philox_ref.normals_f64 forms them."""
    w = np.asarray(words).astype(np.uint64)
    bits = (w[..., 0] << np.uint64(21)) ^ (w[..., 1] >> np.uint64(11))
    u1 = (bits.astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = (w[..., 2].astype(np.float64) + w[..., 3].astype(np.float64) * 2.0 ** -32) * 2.0 ** -32
    return u1, u2


def ln_fixed(u1):
    """ln of a normal positive double: u1 = m 2^e, m in [sqrt(1/2), sqrt 2), the series in s = f / (2 + f), f = m - 1."""
    m, e = np.frexp(u1)  # m in [1/2, 1), exact
    low = m < 0.7071067811865476
    m = np.where(low, m * 2.0, m)
    dk = (e - low).astype(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    q = z * z
    t1 = q * (LG[1] + q * (LG[3] + q * LG[5]))
    t2 = z * (LG[0] + q * (LG[2] + q * (LG[4] + q * LG[6])))
    R = t2 + t1
    hfsq = (0.5 * f) * f
    return (((s * (hfsq + R) + dk * LN2_LO) - hfsq) + f) + dk * LN2_HI


def cos_sin_fixed(u2):
    """(cos, sin) of 2 pi u2: x = 2 u2 half turns, j the nearest quarter turn, t = x - j / 2, y = pi t, the two kernels, the quadrant."""
    x = 2.0 * u2
    jf = np.floor(2.0 * x + 0.5)
    t = x - 0.5 * jf
    y = t * 3.141592653589793
    y2 = y * y
    y3 = y2 * y
    rs = S[1] + y2 * (S[2] + y2 * (S[3] + y2 * (S[4] + y2 * S[5])))
    sn = y + y3 * (S[0] + y2 * rs)
    rc = y2 * (CC[0] + y2 * (CC[1] + y2 * (CC[2] + y2 * (CC[3] + y2 * (CC[4] + y2 * CC[5])))))
    hz = 0.5 * y2
    wc = 1.0 - hz
    cs = wc + (((1.0 - wc) - hz) + y2 * rc)
    j = jf.astype(np.int64) & 3
    c = np.select([j == 0, j == 1, j == 2], [cs, -sn, -cs], sn)
    s = np.select([j == 0, j == 1, j == 2], [sn, cs, -sn], -cs)
    return c, s


def normals(words):
    """Box-Muller's pair from four words, by the fixed sequences."""
    u1, u2 = uniforms(words)
    r = np.sqrt(-2.0 * ln_fixed(u1))
    c, s = cos_sin_fixed(u2)
    return np.stack([r * c, r * s], axis=-1)


def _block(rows, width, seed, attempt, tag):
    seed, attempt = int(seed), int(attempt)
    if not (0 <= seed < 1 << 64 and 0 <= attempt < 1 << 32):
        raise ValueError("seed is 64 bits and the attempt 32")
    groups = -(-width // 2)
    w = pr.philox4x32_10(np.arange(rows)[:, None], np.arange(groups)[None, :], attempt, tag, seed & 0xFFFFFFFF, seed >> 32)
    return normals(w).reshape(rows, 2 * groups)[:, :width]


def draw(K, Z, seed, attempt):
    """(pref_val [K, Z], order_key [K]) of (seed, attempt)."""
    return _block(K, Z, seed, attempt, TAG_PREF), _block(K, 1, seed, attempt, TAG_KEY)[:, 0]


def tables(pref_val, order_key):
    """rank: ascending order_key, ties to the lower user; pref[k]: descending pref_val[k], ties to the lower slot."""
    return np.argsort(order_key, kind="stable"), np.argsort(-pref_val, axis=1, kind="stable")


def reference(Z, state, seed, nattempt):
    """Every attempt through the reference's own greedy on the restated draw: slots [nattempt, K] with -1 = left over, and the counts."""
    K = state[0].shape[0]
    slots, rem = [], []
    for a in range(nattempt):
        rank, pref = tables(*draw(K, Z, seed, a))
        z_vec, _, un = gm_restate.max_rand(Z, state, rank, pref, randint=lambda n, size: np.full(size, -1))
        slots.append(z_vec.astype(np.int64))
        rem.append(int(un))
    return np.stack(slots), rem


def pick_of(rem, rule):
    """Rule 0: the first attempt that leaves nobody over, else the last.  Rule 1: the fewest left over, ties to the lower attempt."""
    if rule == 0:
        return next((a for a, r in enumerate(rem) if r == 0), len(rem) - 1)
    return int(np.argmin(rem))
