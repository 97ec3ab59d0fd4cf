"""Shared by tests/test_fixedpoint_log_host.py and tests/test_gpu_fixedpoint_log.py: the hb_selftest_fxlog runner, the steps on Python
ints, the operands of the end-to-end tests, and an INTEGER enclosure of log_base(x / 2^f) 2^f (digit-by-digit squaring): no float
decides a verdict."""
from fractions import Fraction

import bitdec_cases as bc
import division_cases as dc

FIRST, LEVEL, POLY_MASK, FINISH = range(4)
E = "e"
DEGREES = (2, 3, 5, 8, 13)


# ---- the shape of the levels, restated ------------------------------------------------------------------------------------------
def levels(d):
    """ceil(log2 d)"""
    n = 0
    while (1 << n) < d:
        n += 1
    return n


def level_powers(level, d):
    """the powers level `level` >= 1 forms"""
    half = 1 << (level - 1)
    return [j for j in range(half + 1, 2 * half + 1) if j <= d]


# ---- the enclosure --------------------------------------------------------------------------------------------------------------
def _log2_digits(num, den, digits, up):
    """the first `digits` binary digits of log2(num / den) for 1 <= num / den < 2, as an integer: squaring at 2 digits + 64 bits, every
    squaring rounded down (up = 0: the digits are a lower bound) or up (up = 1: an upper bound once 1 is added in the last place)"""
    w = 2 * digits + 64
    y = (num << w) // den + (up if (num << w) % den else 0)
    out = 0
    for _ in range(digits):
        sq = y * y
        y = (sq >> w) + (up if sq & ((1 << w) - 1) else 0)
        out <<= 1
        if y >> (w + 1):
            out |= 1
            y = (y >> 1) + (up & y & 1)
    return out + up


def log2_enclosure(num, den, digits):
    """-> (lo, hi) Fractions with lo <= log2(num / den) <= hi, 2^(1-digits) apart at the most, for positive integers num, den"""
    e = 0
    while num >= 2 * den:
        den, e = 2 * den, e + 1
    while num < den:
        num, e = 2 * num, e - 1
    return e + Fraction(_log2_digits(num, den, digits, 0), 1 << digits), e + Fraction(_log2_digits(num, den, digits, 1), 1 << digits)


_BASE_CACHE = {}


def _log2_base(base, digits):
    """an enclosure of log2(base); E from sum 1 / n! with its remainder, below 2 / (N + 1)!"""
    key = (base, digits)
    if key not in _BASE_CACHE:
        if base == E:
            total, fact, n = Fraction(0), 1, 0
            while fact.bit_length() < 2 * digits + 80:
                total += Fraction(1, fact)
                n += 1
                fact *= n
            lo, hi = total, total + Fraction(2, fact)
            _BASE_CACHE[key] = (log2_enclosure(lo.numerator, lo.denominator, digits)[0], log2_enclosure(hi.numerator, hi.denominator, digits)[1])
        else:
            _BASE_CACHE[key] = log2_enclosure(base, 1, digits)
    return _BASE_CACHE[key]


def log_enclosure(x, f, base=2):
    """-> (lo, hi) Fractions around log_base(x / 2^f) 2^f, in ulps of 2^-f, from 2 f + 64 digits: f + 64 guard bits"""
    digits = 2 * f + 64
    lo, hi = log2_enclosure(x, 1 << f, digits)
    if base != 2:
        blo, bhi = _log2_base(base, digits)
        lo, hi = (lo / bhi if lo >= 0 else lo / blo), (hi / blo if hi >= 0 else hi / bhi)
    return lo * (1 << f), hi * (1 << f)


def distance(value, enclosure):
    """how far the integer `value` can be from the enclosed number"""
    return max(abs(value - enclosure[0]), abs(value - enclosure[1]))


def centered(v, p):
    return v - p if v > p // 2 else v


# ---- operands -------------------------------------------------------------------------------------------------------------------
def r1_extremes(limits):
    """all-zero and all-ones r1 for every truncation: the two ends of what trunc_pr can add"""
    return [[0] * len(limits), [(1 << m) - 1 for m in limits]]


def e2e_inputs(rnd, k, f, count):
    """at least `count` operands: 0, 1, 2^f (exactly 0 for base 2) and its neighbours, the largest, a power of two at every second bit
    (all of them, so k = 64 gives 37), and random values of random lengths up to `count`"""
    xs = [0, 1, 1 << f, (1 << f) + 1, (1 << f) - 1, (1 << (k - 1)) - 1] + [1 << i for i in range(1, k - 1, 2)]
    while len(xs) < count:
        nb = rnd.randrange(1, k)
        xs.append(rnd.randrange(1 << (nb - 1), 1 << nb))
    return xs


def structured(rnd, k, f, extra):
    """every bit length 1 .. k - 1 at both ends, the neighbours of 2^f, and `extra` random values a length"""
    xs = [1, 1 << f, (1 << f) + 1, (1 << f) - 1, (1 << (k - 1)) - 1]
    for nb in range(1, k):
        xs += [1 << (nb - 1), (1 << nb) - 1] + [rnd.randrange(1 << (nb - 1), 1 << nb) for _ in range(extra)]
    return xs


# ---- the steps on Python ints -----------------------------------------------------------------------------------------------------
def first_on_ints(p, opened, ta, tb, tab, ybig, na, nb, count):
    """-> (masked [2 count], t [count])"""
    t = [(4 * bc.beaver(opened[i], opened[count + i], ta[i], tb[i], tab[i], p) - 3 * ybig[i]) % p for i in range(count)]
    return [(t[i] - na[i]) % p for i in range(count)] + [(t[i] - nb[i]) % p for i in range(count)], t


def trunc_on_ints(p, s, opened, m):
    inv = pow(2, -m, p)
    return [(a - c % (1 << m)) * inv % p for a, c in zip(s, opened)]


def level_on_ints(p, level, d, opened, s, m, ta, tb, powers, count):
    """-> (masked [2 next count], powers [d count] updated)"""
    half = 1 << (level - 1)
    powers = list(powers)
    new = trunc_on_ints(p, s, opened, m)
    for q in range(len(level_powers(level, d))):
        powers[(half + q) * count:(half + q + 1) * count] = new[q * count:(q + 1) * count]
    masked = []
    for q in range(len(level_powers(level + 1, d))):
        masked += [(powers[(2 * half - 1) * count + i] - ta[q * count + i]) % p for i in range(count)]
        masked += [(powers[q * count + i] - tb[q * count + i]) % p for i in range(count)]
    return masked, powers


def poly_mask_on_ints(p, d, opened, s, m_in, powers, ybig, coef, bits, width, m_out, kappa, count):
    """-> (masked [count], s_out [count])"""
    last = levels(d)
    half = 1 << (last - 1)
    powers = list(powers)
    new = trunc_on_ints(p, s, opened, m_in)
    for q in range(len(level_powers(last, d))):
        powers[(half + q) * count:(half + q + 1) * count] = new[q * count:(q + 1) * count]
    nbits = width + kappa
    masked, kept = [], []
    for i in range(count):
        poly = (coef[0] * ybig[i] + sum(coef[j] * powers[(j - 1) * count + i] for j in range(1, d + 1))) % p
        r1 = sum(bits[r * count + i] << r for r in range(m_out))
        r2 = sum(bits[r * count + i] << (r - m_out) for r in range(m_out, nbits))
        masked.append((poly + (1 << (width - 1)) + r1 + (r2 << m_out)) % p)
        kept.append((poly + r1) % p)
    return masked, kept


def finish_on_ints(p, opened, s, m, ipart):
    return [(t + i) % p for t, i in zip(trunc_on_ints(p, s, opened, m), ipart)]


# ---- the bodies on the host ---------------------------------------------------------------------------------------------------
def run_log(p, nl, what, operands, params, outs, count):
    """hb_selftest_fxlog over lists of ints: params as the header lists them -> (rc, [out lists])"""
    return bc._run("hb_selftest_fxlog", 5, p, nl, what, operands, params, outs, count)


ok = dc.ok


# ---- GPU side -------------------------------------------------------------------------------------------------------------------
def selftest_on_tensors(ctx, what, operands, params, out_rows, count, preset=()):
    """hb_selftest_fxlog over the limbs of device tensors (None: absent; a list of ints: constants in host memory), no Python ints in
    between -> [(rows, count, limbs) int64 tensors on the host], one an entry of out_rows (0: absent); preset: {index of an out: a
    tensor it starts from} for the arrays a step updates in place"""
    import ctypes

    import numpy as np

    from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

    p, nl = ctx.modulus, ctx.n_limbs
    preset = dict(preset)
    keep = [None if o is None else (ints_to_limbs(list(o), p, 8 * nl) if isinstance(o, list) else np.ascontiguousarray(o.cpu().numpy())) for o in operands]
    ptrs = (ctypes.c_void_p * 8)(*([None if a is None else a.ctypes.data for a in keep] + [None] * (8 - len(keep))))
    outs = [np.zeros((max(r * count, 1), nl), dtype=np.int64) if r else None for r in out_rows]
    for i, t in preset.items():
        outs[i][:out_rows[i] * count] = t.cpu().numpy().reshape(-1, nl)
    optrs = (ctypes.c_void_p * 2)(*([None if o is None else o.ctypes.data for o in outs] + [None] * (2 - len(outs))))
    prm = (ctypes.c_int64 * 5)(*(list(params) + [0] * (5 - len(params))))
    rc = load_library().hb_selftest_fxlog(np_ptr(ints_to_limbs([p], p + 1, 8 * nl)), nl, what, ptrs, prm, optrs, count)
    assert rc == 0, rc
    return [None if o is None else ctx.torch.from_numpy(o[:r * count]).view(r, count, nl) for o, r in zip(outs, out_rows)]


def truncation_planes(lay, kappa):
    """-> [first plane of every truncation in step order] from a log_layout"""
    nb = lay["width"] + kappa
    starts = []
    for name, (start, stop) in sorted(lay["planes"].items(), key=lambda kv: kv[1]):
        if name != "bit_decompose":
            starts += list(range(start, stop, nb))
    return starts
