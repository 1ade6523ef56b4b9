"""The device Gaussian generator restated in NumPy, from its definition ("The generator as a contract").

Nothing here is taken from the kernels: Philox4x32-10 follows Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as
1, 2, 3" (SC'11) -- test_sketch_rng_host.py holds it to Random123's published vectors -- and the normals follow the two Box-Muller
forms the contract states.  Everything is vectorised over the leading axes; the four words of a draw sit on the last axis.

    philox4x32_10(c0, c1, c2, c3, k0, k1)  -> uint32 [..., 4]
    normals_f64(words)                      -> float64 [..., 2]   one 53-bit and one 64-bit uniform
    normals_f32(words, ftype)               -> ftype   [..., 4]   four 24-bit uniforms, evaluated in np.float64 or np.float32
    sketch(K, D, seed, iteration, dtype)    -> float64 [K, D]     the block of an MMW iteration, dtype "f64" | "f32" (| "f32-in-f32")
    randv(Z, Dp, seed, attempt)             -> float64 [Z, Dp]    the rounding's directions of one attempt
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57   # the round's two multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # the key schedule's Weyl increments (golden ratio, sqrt(3) - 1)
TAG_SKETCH = 0x4D4D5753           # "MMWS"
TAG_RANDV = 0x524E4456            # "RNDV"
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox-4x32 on the counter (c0, c1, c2, c3) under the key (k0, k1); arguments broadcast.  A round maps
    (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) and then bumps the key by (W0, W1)."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k = [np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)]
    sh = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 bits: fits 64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & MASK, (p0 >> sh) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def normals_f64(words):
    """Two standard normals from four words: u1 = ((w0 << 21 ^ w1 >> 11) + 1) 2^-53 in (0, 1], u2 = (w2 + w3 2^-32) 2^-32 in [0, 1),
    r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2)."""
    w = np.asarray(words).astype(np.uint64)
    bits = (w[..., 0] << np.uint64(21)) ^ (w[..., 1] >> np.uint64(11))  # 53 bits: exact in a double, and so is the + 1
    u1 = (bits.astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = (w[..., 2].astype(np.float64) + w[..., 3].astype(np.float64) * 2.0 ** -32) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=-1)


def normals_f32(words, ftype=np.float64):
    """Four standard normals from four words, the fp32 form: radii from the 24-bit uniforms ((w >> 8) + 1) 2^-24 in (0, 1] of w0 and
    w2, angles from (w >> 8) 2^-24 in [0, 1) of w1 and w3, r = sqrt(-2 ln2 log2 u); (r1 cos, r1 sin, r2 cos, r2 sin).  `ftype`:
    np.float64 evaluates the formula exactly enough to be the reference; np.float32 rounds every step to fp32 with correctly
    rounded functions -- what a faithful fp32 implementation could give, the yardstick of the device's error."""
    f = np.dtype(ftype).type
    t = np.asarray(words).astype(np.uint32) >> np.uint32(8)
    ur = ((t[..., 0::2] + np.uint32(1)).astype(ftype)) * f(2.0 ** -24)  # 24-bit integers: exact in either type
    ua = t[..., 1::2].astype(ftype) * f(2.0 ** -24)
    r = np.sqrt(f(-2.0 * np.log(2.0)) * np.log2(ur))
    a = f(2.0 * np.pi) * ua
    out = np.empty(t.shape, dtype=ftype)
    out[..., 0::2] = r * np.cos(a)
    out[..., 1::2] = r * np.sin(a)
    return out


def _draw(rows, width, per, seed, index, tag, normals):
    """[rows, width] normals before normalisation: group p of a row is the draw of counter (row, p, index, tag) under the key (seed
    low word, seed high word) and holds the columns per p ... per p + per - 1; columns >= width do not count."""
    seed = int(seed)
    if not (0 <= seed < 1 << 64 and 0 <= int(index) < 1 << 32):
        raise ValueError("seed is 64 bits and the iteration / attempt 32")
    groups = -(-width // per)
    w = philox4x32_10(np.arange(rows)[:, None], np.arange(groups)[None, :], int(index), tag, seed & 0xFFFFFFFF, seed >> 32)
    return normals(w).reshape(rows, groups * per)[:, :width]


def _unit_rows(n):
    n = np.asarray(n)
    return n / np.sqrt(np.sum(n * n, axis=1, dtype=n.dtype))[:, None]


def sketch(K, D, seed, iteration, dtype="f64"):
    """The row-normalised K x D block of `iteration` of a run with `seed`, float64.  dtype "f64": pairs of columns from normals_f64;
    "f32": quadruples from normals_f32 evaluated in float64 (the reference of an fp32 handle); "f32-in-f32": the same evaluated and
    normalised in np.float32 (the yardstick)."""
    if dtype == "f64":
        return _unit_rows(_draw(K, D, 2, seed, iteration, TAG_SKETCH, normals_f64))
    if dtype == "f32":
        return _unit_rows(_draw(K, D, 4, seed, iteration, TAG_SKETCH, normals_f32))
    if dtype == "f32-in-f32":
        n = _draw(K, D, 4, seed, iteration, TAG_SKETCH, lambda w: normals_f32(w, np.float32))
        return _unit_rows(n).astype(np.float64)
    raise ValueError("dtype is f64, f32 or f32-in-f32")


def randv(Z, Dp, seed, attempt):
    """The row-normalised Z x Dp directions of rounding attempt `attempt` with `seed`: the fp64 form under the rounding's tag."""
    return _unit_rows(_draw(Z, Dp, 2, seed, attempt, TAG_RANDV, normals_f64))


def sketch_f32_yardstick(K, D, seed, iteration):
    """e_ref of a case: max |sketch evaluated in float32 - sketch evaluated in float64| on the same words."""
    return float(np.max(np.abs(sketch(K, D, seed, iteration, "f32-in-f32") - sketch(K, D, seed, iteration, "f32"))))
