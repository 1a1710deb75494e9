"""Primitive level: the device text of numeric contract HJ-NUM-1 (kernels/hj_num.h, through hj_debug_num) against the oracle's text
(oracle/hj_oracle.c, through hjo_num_batch) on chosen inputs, 0 differing bits.  One exception: a NaN equals any NaN - sign and
payload of a generated NaN are outside the contract, and x86 and the GPU produce different defaults.

Per op the inputs are: every binade with stratified mantissas; +-0, +-inf, NaN, the smallest and largest denormals; one and two ulps
each side of every constant the text branches on; for the binary ops the cross product of a list of special values (both orders of
the two zeros, a NaN in either place); for the RNG ops 2^20 states, among them the states whose first or second draw is 0 (none but state
0), 1, 0xFFFFFF7F (the largest value below 1.0f), 0xFFFFFF80 (the smallest that rounds to 1.0f) and 0xFFFFFFFF - xorshift is
invertible, so they are computed.  The tests without the gpu mark check these premises with the oracle alone.

sincos2pi is compared over every binade too: where |rint(4v)| reaches 2^31 the quadrant is the saturated conversion's, which C
leaves undefined and the contract therefore spells out.  Signalling NaNs are left out: the contract speaks
of quiet ones."""
import ctypes as C
import functools

import numpy as np
import pytest

import fuzz_cases
from hijiki_amd import abi, device

U = np.uint32

# which words of an op's 4 output words are floats (a NaN there equals any NaN); every other word is compared as an integer
FLOAT_WORDS = {"exp": 1, "sincos2pi": 2, "atan2": 1, "asin": 1, "min": 1, "max": 1, "div": 1, "sqrt": 1, "dot3": 1, "cross3": 3,
               "normalize3": 3, "reflect3": 3, "rng_seed": 0, "rng_uint": 0, "rng_float": 1, "rand_cos_hemisphere": 3,
               "rand_uniform_sphere": 3, "rand_barycentric": 3}
assert tuple(FLOAT_WORDS) == abi.NUM_OPS

SPECIALS = U([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345,     # +-0, +-inf, quiet NaNs
              0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,   # denormals, FLT_MIN, FLT_MAX
              0x3F800000, 0xBF800000, 0x3F7FFFFF, 0x3F800001, 0xBF7FFFFF, 0xBF800001, 0x3F000000, 0xBF000000, 0x40000000, 0xC0000000,
              0x1E3CE508, 0x9E3CE508, 0x60AD78EC, 0xE0AD78EC])                                          # +-1e-20, +-1e20
RNG_TARGETS = U([1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x00000080, 0x00000100, 0xFFFFFF00, 0x40000000, 0xC0000000])


def words(x):
    return np.ascontiguousarray(x, np.float32).view(U)


def around(values, k=2):
    """The float32 nearest every value and its k neighbours each side."""
    w = words(np.atleast_1d(np.asarray(values, np.float64)).astype(np.float32)).astype(np.int64)
    return (w[:, None] + np.arange(-k, k + 1)[None, :]).ravel().astype(U)


def binades(rng, per=32, lo=0, hi=254):
    """Both signs of every binade lo .. hi (0: the denormals): its first and last value and `per` stratified mantissas."""
    e = np.arange(lo, hi + 1, dtype=np.int64)
    step = (1 << 23) // per
    m = np.arange(per, dtype=np.int64)[None, :] * step + rng.integers(0, step, (len(e), per))
    m = np.concatenate([m, np.zeros((len(e), 1), np.int64), np.full((len(e), 1), 0x7FFFFF, np.int64)], axis=1)
    w = ((e[:, None] << 23) | m).ravel()
    w = w[w != 0]
    return np.concatenate([w, w | 0x80000000]).astype(U)


def cross(a, b=None):
    b = a if b is None else b
    return np.stack([np.repeat(a, len(b)), np.tile(b, len(a))], axis=1)


def unxorshift(x):
    """The state whose next rng_uint is x: s ^= s << 13, s ^= s >> 17, s ^= s << 5 undone from the back."""
    x = np.asarray(x, np.uint64)
    M = np.uint64(0xFFFFFFFF)

    def undo(y, shift, left):
        s = y.copy()
        for _ in range(32 // shift + 1):
            s = y ^ (((s << np.uint64(shift)) & M) if left else (s >> np.uint64(shift)))
        return s
    return undo(undo(undo(x, 5, True), 17, False), 13, True).astype(U)


def rng_states(rng, n):
    """n states: the chosen ones, filled up with random ones."""
    first = unxorshift(RNG_TARGETS)
    chosen = np.concatenate([np.arange(256, dtype=U), U([0xFFFFFFFF, 0x80000000]), first, unxorshift(first)])
    return np.concatenate([rng.integers(0, 1 << 32, n - len(chosen), dtype=np.uint64).astype(U), chosen])


def vectors(rng):
    """(n, 6) words: two 3-vectors per record."""
    n = 1 << 15
    plain = rng.normal(size=(2 * n, 6)).astype(np.float32)
    mixed = (rng.normal(size=(2 * n, 6)) * np.exp2(rng.integers(-40, 41, (2 * n, 6)))).astype(np.float32)       # cancellation, lost terms
    wide = rng.choice(binades(rng, 4), (n, 6))                                                          # overflow, denormal products
    pick = np.concatenate([SPECIALS, words([0.3, 3.0, -0.3, -3.0])])
    special = rng.choice(pick, (n, 6))
    # unit vectors scaled to the lengths the integrator really produces (0 .. 1e20), and with a component zeroed
    d = rng.normal(size=(n // 4, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    nrm = rng.normal(size=(n // 4, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    scaled = [np.concatenate([(d * s).astype(np.float32), nrm.astype(np.float32)], axis=1) for s in (0.0, 1e-20, 0.3, 3.0, 1e20)]
    for c in range(3):
        z = d.copy()
        z[:, c] = 0.0 if c < 2 else -0.0
        scaled.append(np.concatenate([z.astype(np.float32), nrm.astype(np.float32)], axis=1))
    tangent = np.cross(d, nrm)                                                                          # I perpendicular to N up to rounding
    scaled.append(np.concatenate([tangent.astype(np.float32), nrm.astype(np.float32)], axis=1))
    axes = np.eye(3, dtype=np.float32)[rng.integers(0, 3, (n // 4, 2))].reshape(-1, 6) * rng.choice([1.0, -1.0, 0.0], (n // 4, 6)).astype(np.float32)
    return np.concatenate([words(plain), words(mixed), wide, special, words(np.concatenate(scaled)), words(axes)])


@functools.lru_cache(maxsize=None)
def inputs(op):
    """The (n, k) uint32 input words of `op`, a function of fuzz_cases.source_seed() alone."""
    rng = np.random.default_rng([fuzz_cases.source_seed(), abi.NUM_OPS.index(op)])
    n = 1 << 18
    ln2 = np.log(2.0)
    if op == "exp":
        cuts = (np.arange(-127, 129) + 0.5) * ln2                                                       # where rint(x log2 e) steps
        w = np.concatenate([binades(rng), SPECIALS, around([-87.0, 88.0, 0.0, -104.0]), around(cuts), words(rng.uniform(-104.5, 89.5, n)),
                            words(rng.uniform(-1.0, 1.0, n // 4))])
    elif op == "sincos2pi":
        quarters = np.arange(-16, 17) / 4.0
        w = np.concatenate([binades(rng), SPECIALS, around(quarters), around(quarters + 0.125), words(rng.uniform(0.0, 1.0, n)),
                            words(rng.uniform(-4.0, 4.0, n // 4)), words(rng.integers(0, 1 << 32, n // 4).astype(np.float32) * np.float32(2.0 ** -32))])
        w = np.concatenate([w, around([2.0 ** 29, -2.0 ** 29, 2.0 ** 21, -2.0 ** 21])])                     # (int)k saturates; rint(4v) by the magic constant ends
    elif op == "asin":
        w = np.concatenate([binades(rng), SPECIALS, around([0.5, -0.5, 1.0, -1.0]), words(rng.uniform(-1.0, 1.0, n)),
                            words(1.0 - rng.uniform(0.0, 1.0, n // 4) ** 4)])
    elif op == "sqrt":
        w = np.concatenate([binades(rng), SPECIALS, words(rng.uniform(0.0, 4.0, n)), rng.integers(0, 0x7F800000, n).astype(U)])
    elif op in ("min", "max"):
        b = binades(rng, 4)
        same = rng.choice(b, 4096)
        w = np.concatenate([cross(SPECIALS), cross(rng.choice(b, 256), SPECIALS), cross(SPECIALS, rng.choice(b, 256)),
                            rng.choice(b, (n // 4, 2)), np.stack([same, same], axis=1), np.stack([same, same ^ U(0x80000000)], axis=1)])
    elif op == "div":
        b = binades(rng, 8)
        w = np.concatenate([cross(SPECIALS), cross(rng.choice(b, 256), SPECIALS), cross(SPECIALS, rng.choice(b, 256)), rng.choice(b, (n, 2)),
                            words(rng.normal(size=(n, 2))), rng.integers(1, 1 << 24, (n // 4, 2)).astype(np.float32).view(U)])
    elif op == "atan2":
        b = binades(rng, 8)
        x = (rng.normal(size=4096) * np.exp2(rng.integers(-30, 31, 4096))).astype(np.float32)
        near = []
        for c in (0.4142135623730950, 2.414213562373095, 1.0):                                          # the cuts of hj_atan_pos, and y == x
            yw = words(np.float32(c) * np.abs(x)).astype(np.int64)
            for off in range(-3, 4):
                y = (yw + off).astype(U) | (rng.integers(0, 2, len(x)).astype(U) << U(31))
                near.append(np.stack([y, words(x)], axis=1))
        w = np.concatenate([cross(SPECIALS), cross(rng.choice(b, 256), SPECIALS), cross(SPECIALS, rng.choice(b, 256)), *near,
                            words(rng.normal(size=(n, 2))), rng.choice(b, (n // 4, 2))])
    elif op in ("dot3", "cross3", "normalize3", "reflect3"):
        w = vectors(rng)
    elif op == "rng_seed":
        chosen = np.concatenate([np.arange(1 << 16, dtype=U), U([61, 0xFFFFFFFF, 0x80000000])])
        w = np.concatenate([rng.integers(0, 1 << 32, (1 << 20) - len(chosen), dtype=np.uint64).astype(U), chosen])
    else:
        w = rng_states(rng, 1 << 20)
    w = np.ascontiguousarray(w.reshape(len(w), -1))
    assert len(w) <= abi.NUM_MAX_RECORDS
    return w


def mismatches(op, got, want):
    """Rows of two (n, 4) uint32 results that differ: bit for bit, but in an op's float words a NaN equals any NaN."""
    same = got == want
    k = FLOAT_WORDS[op]
    if k:
        same[:, :k] |= np.isnan(got[:, :k].view(np.float32)) & np.isnan(want[:, :k].view(np.float32))
    return np.flatnonzero(~same.all(axis=1))


def report(op, w, got, want, bad):
    lines = [f"{op}: {len(bad)} of {len(w)} records differ (HJ_FUZZ_SEED={fuzz_cases.source_seed()})"]
    for i in bad[:12]:
        lines.append("  in " + " ".join(f"{v:08x}" for v in w[i]) + "  device " + " ".join(f"{v:08x}" for v in got[i])
                     + "  oracle " + " ".join(f"{v:08x}" for v in want[i]))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ premises (no GPU)

def test_inputs_hold_what_the_tests_claim(oracle):
    """The premises of the GPU comparison, from the oracle alone: the input sets hold the special values and both sides of every
    constant the texts branch on, and enough records take each branch."""
    def has(op, values, col=0):
        col_words = inputs(op)[:, col]
        for v in values:
            assert (col_words == words([v])[0]).any(), (op, v)
    for op in ("exp", "sincos2pi", "asin", "sqrt"):
        assert np.isin(SPECIALS[:13], inputs(op)[:, 0]).all(), op
        e = (inputs(op)[:, 0] >> U(23)) & U(0xFF)
        assert len(np.unique(e)) == 256, (op, len(np.unique(e)))
    for c in (-87.0, 88.0):
        has("exp", [c, np.nextafter(np.float32(c), np.float32(-np.inf)), np.nextafter(np.float32(c), np.float32(np.inf))])
    has("asin", [0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)), 1.0, -1.0])
    for k in range(0, 5):
        has("sincos2pi", [k / 4.0, np.nextafter(np.float32(k / 4.0), np.float32(-9)), np.nextafter(np.float32(k / 4.0), np.float32(9))])
    # sincos2pi: finite arguments whose k = rint(4v) is outside int's range, both signs, and the last k inside it (2^31 - 256: the sum with
    # the magic constant has an ulp of 256 there; -(2^31 - 128)); 0x4DFFFFFF is the v below 2^29 that the sum rounds up to k = 2^31
    v = inputs("sincos2pi")[:, 0].view(np.float32)
    with np.errstate(all="ignore"):
        k = (v * np.float32(4) + np.float32(12582912)) - np.float32(12582912)                           # 4v is exact, so this is the fmaf
    assert (np.isfinite(v) & (k >= 2.0 ** 31)).sum() >= 100 and (np.isfinite(v) & (k <= -2.0 ** 31)).sum() >= 100
    assert (words(k) == 0x4EFFFFFE).any() and (words(k) == 0xCEFFFFFF).any() and (words(v) == 0x4DFFFFFF).any()
    # exp: flushed, denormal-range (none: results below 2^-126 are cut at -87), finite and overflowing results
    out = oracle.num_batch("exp", inputs("exp"))[:, 0].view(np.float32)
    x = inputs("exp")[:, 0].view(np.float32)
    assert ((out == 0) & (x > -104) & (x < -86)).sum() >= 100 and np.isinf(out).sum() >= 100 and (np.isfinite(out) & (out > 0)).sum() >= 100000
    # atan2: both cuts of hj_atan_pos from both sides, every quadrant, exact zeros in either place
    a = inputs("atan2").view(np.float32)
    with np.errstate(all="ignore"):
        q = np.abs(a[:, 0]) / np.abs(a[:, 1])
    for c in (np.float32(0.4142135623730950), np.float32(2.414213562373095)):
        assert ((q > c) & (q < c * np.float32(1.000001))).sum() >= 100 and ((q <= c) & (q > c * np.float32(0.999999))).sum() >= 100
    for sy in (0, 1):
        for sx in (0, 1):
            sel = ((inputs("atan2")[:, 0] >> U(31)) == sy) & ((inputs("atan2")[:, 1] >> U(31)) == sx)
            assert (sel & (a[:, 0] == 0) & (a[:, 1] == 0)).sum() >= 1 and (sel & (a[:, 0] == 0) & (a[:, 1] != 0)).sum() >= 1
            assert (sel & (a[:, 0] != 0) & (a[:, 1] == 0)).sum() >= 1 and (sel & np.isfinite(q) & (q > 0)).sum() >= 100
    # min / max: both orders of the two zeros, a NaN in either place and in both
    for op in ("min", "max"):
        w = inputs(op)
        assert ((w[:, 0] == 0) & (w[:, 1] == 0x80000000)).any() and ((w[:, 0] == 0x80000000) & (w[:, 1] == 0)).any()
        na, nb = np.isnan(w[:, 0].view(np.float32)), np.isnan(w[:, 1].view(np.float32))
        assert (na & ~nb).sum() >= 100 and (~na & nb).sum() >= 100 and (na & nb).sum() >= 1
    # the RNG: the computed states really draw the targets, first and second; rng_float reaches exactly 1.0 and the value below it
    s = unxorshift(RNG_TARGETS)
    assert (oracle.num_batch("rng_uint", s)[:, 0] == RNG_TARGETS).all()
    assert (oracle.num_batch("rng_uint", oracle.num_batch("rng_uint", unxorshift(s))[:, 1])[:, 0] == RNG_TARGETS).all()
    assert np.isin(s, inputs("rng_float")[:, 0]).all() and np.isin(unxorshift(s), inputs("rand_barycentric")[:, 0]).all()
    f = oracle.num_batch("rng_float", inputs("rng_float"))[:, 0].view(np.float32)
    assert (f == 1.0).sum() >= 2 and (f == np.nextafter(np.float32(1), np.float32(0))).sum() >= 1 and (f == 0.0).sum() == 1
    # rand_barycentric: the fold u + v > 1 taken and not; rand_cos_hemisphere with u == 1 (z = sqrt(max(0, 1 - u)) = 0)
    bw = inputs("rand_barycentric")[:, 0]
    d1 = oracle.num_batch("rng_float", bw)
    d2 = oracle.num_batch("rng_float", d1[:, 1])
    folded = d1[:, 0].view(np.float32) + d2[:, 0].view(np.float32) > 1.0
    assert folded.sum() >= 100000 and (~folded).sum() >= 100000
    assert (oracle.num_batch("rand_cos_hemisphere", inputs("rand_cos_hemisphere"))[:, 2] == 0).sum() >= 2
    # the vectors: zero, tiny and huge lengths, NaN and inf components
    v = inputs("normalize3")[:, :3].view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        ln = np.sqrt((v * v).sum(axis=1))
    assert (ln == 0).sum() >= 100 and ((ln > 0) & (ln < 1e-19)).sum() >= 100 and (np.isfinite(ln) & (ln > 1e19)).sum() >= 100
    assert np.isnan(ln).sum() >= 100 and np.isinf(ln).sum() >= 100


def test_batch_is_the_text_the_scalar_probes_export(oracle):
    """hjo_num_batch calls the same functions as the scalar exports the accuracy tests use (tests/test_oracle_math.py)."""
    L = oracle.lib()
    rng = np.random.default_rng(5)
    x = rng.uniform(-90, 90, 500).astype(np.float32)
    got = oracle.num_batch("exp", words(x))[:, 0]
    assert (got == words([L.hjo_exp(float(v)) for v in x])).all()
    y = rng.normal(size=(500, 2)).astype(np.float32)
    got = oracle.num_batch("atan2", words(y))[:, 0]
    assert (got == words([L.hjo_atan2(float(a), float(b)) for a, b in y])).all()
    out = (C.c_float * 3)()
    for s0 in (1, 12345, 0xDEADBEEF):
        st = C.c_uint32(s0)
        L.hjo_cos_hemisphere(C.byref(st), out)
        got = oracle.num_batch("rand_cos_hemisphere", U([s0]))[0]
        assert (got[:3] == words(list(out))).all() and got[3] == st.value
    assert L.hjo_num_batch(len(abi.NUM_OPS), None, 0, None) == abi.HJ_ERR_INVALID


def test_min_max_known_answers(oracle):
    """HJ-NUM-1's min / max: minNum / maxNum - a quiet NaN loses against a number - and -0 < +0 in either
    argument order, which is what v_min_f32 / v_max_f32 answer.  minNum itself leaves the zero's sign open; the oracle's first
    text returned its second argument there."""
    P0, N0, ONE, NAN = 0x00000000, 0x80000000, 0x3F800000, 0x7FC00000
    pairs = U([[P0, N0], [N0, P0], [P0, P0], [N0, N0], [NAN, ONE], [ONE, NAN], [NAN, N0], [N0, NAN], [ONE, N0], [0xBF800000, P0]])
    assert oracle.num_batch("min", pairs)[:, 0].tolist() == [N0, N0, P0, N0, ONE, ONE, N0, N0, N0, 0xBF800000]
    assert oracle.num_batch("max", pairs)[:, 0].tolist() == [P0, P0, P0, N0, ONE, ONE, N0, N0, ONE, P0]
    assert np.isnan(oracle.num_batch("min", U([[NAN, 0xFFC00000]]))[:, 0].view(np.float32)).all()


def test_sincos2pi_known_answers_outside_int(oracle):
    """HJ-NUM-1's float -> int saturates and sends a NaN to 0, as v_cvt_i32_f32 does; C leaves it undefined
    and x86 answers INT32_MIN throughout.  hj_sincos2pi's quadrant is ((int)k) & 3, so from |k| = 2^31 on it is 3 for a positive
    and 0 for a negative argument.  0x4DFFFFFF is the largest v with 4v < 2^31, but adding the magic constant rounds its k to 2^31."""
    P0, ONE, MONE = 0x00000000, 0x3F800000, 0xBF800000
    v = U([0x4E800000, 0xCE800000, 0x71800000, 0xF1800000, 0x4DFFFFFE, 0x4DFFFFFF, 0xCDFFFFFF, 0xCE000000])   # +-2^30, +-2^100, 2^29 - 64, +-(2^29 - 32), -2^29
    want = [[MONE, P0], [P0, ONE], [MONE, P0], [P0, ONE],                    # r = +0, so (s, c) = (+0, 1); q = 3 gives (-c, s), q = 0 (s, c)
            [P0, ONE],                                                       # k = 2^31 - 256, the last inside int
            [0xD66D10BA, 0x5416BB68],                                        # k = 2^31, r = -32: (-c, s) of the polynomials far outside their range
            [P0, ONE], [P0, ONE]]                                            # k = -(2^31 - 128) and -2^31 = INT32_MIN itself: q = 0
    assert oracle.num_batch("sincos2pi", v)[:, :2].tolist() == want


# ------------------------------------------------------------------------------------------------------- the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("op", abi.NUM_OPS)
def test_device_primitive_equals_oracle(op, gpu_renderer, oracle):
    w = inputs(op)
    got = gpu_renderer.num_probe(op, w)
    want = oracle.num_batch(op, w)
    bad = mismatches(op, got, want)
    print(f"{op}: {len(w)} records, {len(bad)} differ")
    assert len(bad) == 0, report(op, w, got, want, bad)


@pytest.mark.gpu
def test_record_counts_and_refusals(gpu_renderer, oracle):
    """Wave tails and more than one block (a block is 256 threads), and every refusal with its status and a message."""
    w = inputs("rand_uniform_sphere")
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        got = gpu_renderer.num_probe("rand_uniform_sphere", w[:n])
        assert len(mismatches("rand_uniform_sphere", got, oracle.num_batch("rand_uniform_sphere", w[:n]))) == 0, n
    L = device.lib()
    h = gpu_renderer._h
    up = C.POINTER(C.c_uint32)
    buf = np.zeros(abi.NUM_IN_WORDS, U)
    p = buf.ctypes.data_as(up)
    for args, text in (((0, p, 0, p), "no records"), ((0, None, 1, p), "null"), ((0, p, 1, None), "null"),
                       ((len(abi.NUM_OPS), p, 1, p), "op"), ((0, p, abi.NUM_MAX_RECORDS + 1, p), "at most")):
        assert L.hj_debug_num(h, *args) == abi.HJ_ERR_INVALID, args
        assert text in L.hj_last_error(h).decode(), (text, L.hj_last_error(h))
    assert L.hj_debug_num(None, 0, p, 1, p) == abi.HJ_ERR_INVALID                          # no context: a status, and nowhere to leave a message
