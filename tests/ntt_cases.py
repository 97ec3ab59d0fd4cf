"""The transform's test cases and their reference, shared by test_ntt_cases_host.py (no GPU) and test_gpu_ntt.py: plain Python ints, no
GPU, no oracle.

csrc/hb_ntt.hip evaluates out[i] = sum_{j < min(d, n)} c[j] omega^(i j), i < k, on one of four routes (hb_debug_fft_route): 0 the
Vandermonde mat-vec, 1 the whole transform in LDS (k_ntt_lds: value-lazy radix-8 passes, input pruning by the exact d), 2 the four-step
transform over it for orders that do not fit, 3 the stage loop over HBM.  Every case below carries the route it expects -- route_model()
is this module's own transcription of the launcher's cost model, and the GPU test holds it against the library's answer before it compares
a value, so a test cannot silently compare another kernel than the one it names.

Fields: one modulus per class of the reduction code (table below); rows(): edge-valued coefficients (edge_values.py)."""
import collections
import functools
import random

import edge_values as ev
from conftest import BLS

Field = collections.namedtuple("Field", "id p n_limbs adicity psc")

# psc: 4 limbs and 2^254 <= p -- k_ntt_lds<9, 8, *, true>, the one-digit Barrett quotient of reduce2p; other 4-limb moduli take the
# generic REDC(x (R mod p)); 1-limb contexts are k_ntt_lds<3, 2>
FIELDS = [
    Field("bls", BLS, 4, 32, True),                                        # the workload's field
    Field("top", (1 << 256) - 268 * (1 << 20) + 1, 4, 22, True),           # next to 2^256: 2^(32 NW) + 24 p < R at its tightest
    Field("psc-lo", (1 << 254) + 143 * (1 << 20) + 1, 4, 20, True),        # the lower edge of PSC: the quotient's largest values
    Field("gen-hi", (1 << 254) - 13 * (1 << 20) + 1, 4, 20, False),        # generic reduce2p, just below the switch
    Field("stark", (1 << 251) + 17 * (1 << 192) + 1, 4, 192, False),       # generic, 252 bits
    Field("w65", (1 << 64) + 6 * (1 << 20) + 1, 4, 21, False),             # the smallest modulus that needs 4 limbs
    Field("tiny-wide", 12289, 4, 12, False),                               # m[u] about 2^256 as a multiple of a 14-bit p
    Field("goldilocks", (1 << 64) - (1 << 32) + 1, 1, 32, False),          # narrow
    Field("n61", (1 << 61) - (1 << 21) + 1, 1, 21, False),                 # narrow, another word shape
    Field("tiny", 12289, 1, 12, False),                                    # narrow, tiny
]
FIELD = {f.id: f for f in FIELDS}

MATVEC, LDS, FOUR_STEP, STAGE_LOOP = 0, 1, 2, 3


def default_limbs(p):
    """the limb count Context.get(p) picks: the fields that want another one are called through the C entry"""
    return 1 if p < 1 << 64 else 4


def root_of_unity(p, order):
    """a root of unity of exact order `order` (a power of two dividing p - 1): a power of the first quadratic non-residue"""
    assert order >= 1 and order & (order - 1) == 0 and (p - 1) % order == 0
    g = next(a for a in range(2, 1000) if pow(a, (p - 1) // 2, p) != 1)
    omega = pow(g, (p - 1) // order, p)
    assert order == 1 or pow(omega, order // 2, p) == p - 1
    return omega


# ---- reference transform ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _powers(p, omega, half):
    tw = [1] * max(half, 1)
    for j in range(1, half):
        tw[j] = tw[j - 1] * omega % p
    return tw


def dft(p, omega, n, coeffs, k=None):
    """the first k of out[i] = sum_j c[j] omega^(i j), i < n: iterative radix-2 decimation in time.  Lists shorter than n are zero
    padded, longer ones truncated to n (the reference does the same, rsdecode_impl.h:173)"""
    assert n >= 1 and n & (n - 1) == 0
    logn = n.bit_length() - 1
    c = [v % p for v in coeffs[:n]] + [0] * (n - min(len(coeffs), n))
    a = [0] * n
    for i in range(n):
        a[int(format(i, "0%db" % logn)[::-1], 2) if logn else 0] = c[i]
    tw = _powers(p, omega, n // 2)
    m = 2
    while m <= n:
        half, step = m // 2, n // m
        w = tw[0 : half * step : step] if half > 1 else [1]
        for s in range(0, n, m):
            lo = a[s : s + half]
            t = [x * y % p for x, y in zip(w, a[s + half : s + m])]
            a[s : s + half] = [(u + v) % p for u, v in zip(lo, t)]
            a[s + half : s + m] = [(u - v) % p for u, v in zip(lo, t)]
        m *= 2
    return a[: n if k is None else k]


def dft_horner(p, omega, n, coeffs, k=None):
    """the definition, for n <= 64"""
    assert n <= 64
    c = [v % p for v in coeffs[:n]]
    out = []
    for i in range(n if k is None else k):
        x, acc = pow(omega, i, p), 0
        for co in reversed(c):
            acc = (acc * x + co) % p
        out.append(acc)
    return out


def inverse_rows(p, omega, n, targets):
    """coefficient rows whose n-point transforms at omega are `targets`"""
    ninv, winv = pow(n, -1, p), pow(omega, -1, p)
    return [[v * ninv % p for v in dft(p, winv, n, row)] for row in targets]


# ---- rows ------------------------------------------------------------------------------------------------------------------------
def rows(p, d, count, seed=0, n_limbs=None):
    """`count` rows of d canonical coefficients after edge_values.edge_rows, over the pool of the CONTEXT's limb count (12289 on 4 limbs
    has its edges at 2^256): walk rows (row k holds pool[(k + 7 i + seed) % len(pool)] at position i, so len(pool) of them put every
    value at every position once) as far as count allows, the all-(p - 1) row, draws from the pool and its Montgomery pre-images, the
    all-zero row and -- with four rows or more -- one uniform row"""
    nl = n_limbs or ev.n_limbs_of(p)
    if nl == ev.n_limbs_of(p) and count - 2 > len(ev.edge_pool(p, nl)) + 1:
        out = ev.edge_rows(p, d, count - 2, seed)              # the whole walk, p - 1, draws
    else:
        pool, pre = ev.edge_pool(p, nl), ev.montgomery_preimages(p, nl)
        rnd = random.Random(seed)
        uniform = 1 if count >= 4 else 0
        n_walk = min(len(pool), max(count - 3 - uniform, 0))
        out = [[pool[(k + 7 * i + seed) % len(pool)] for i in range(d)] for k in range(n_walk)]
        if count >= 1:
            out.append([p - 1] * d)
        while len(out) < count - 1 - uniform:
            out.append([rnd.choice(pre) if rnd.random() < 0.25 else rnd.choice(pool) for _ in range(d)])
    if count >= 2:
        out.append([0] * d)
    if count >= 4:
        rnd = random.Random(seed + 1)
        out.append([rnd.randrange(p) for _ in range(d)])
    assert len(out) == count and all(0 <= v < p for r in out for v in r)
    return out


def half_rows(p, n):
    """for every bit b of the coefficient index: p - 1 where the bit is set and 0 elsewhere, and the complement.  Whatever stage pairs the
    two halves of such a split meets u = 0 against v = the sum of 2^s values p - 1 (and the reverse): the difference u - v + M of the
    first pass's trivial butterflies at its lowest, the sum at its highest, in every remainder pass and on both factors of a four-step"""
    out = []
    for b in range(n.bit_length() - 1):
        out.append([p - 1 if (j >> b) & 1 else 0 for j in range(n)])
        out.append([0 if (j >> b) & 1 else p - 1 for j in range(n)])
    return out


# ---- the launcher's rule, transcribed (hb_ntt.hip, fft_route) -----------------------------------------------------------------------
def lds_pb(n):
    return min(2048 // n, 256) if n <= 2048 else 1


def route_model(n_limbs, n, d, k, stage_loop=False):
    """(route, n1, n2, PB) as hb_debug_fft_route reports it: MADs of the lazily reduced mat-vec against those of the butterflies, then
    what fits the 160 KB of LDS (n data + n / 2 twiddle elements of 9 or 3 digits)"""
    nl = 9 if n_limbs == 4 else 3
    logn, dd = n.bit_length() - 1, min(d, n)
    prod, red = nl * nl, nl * nl + 4 * nl
    if dd == 0 or n == 1 or (k * dd <= 4000000 and 2 * (k * dd * prod + k * red) <= n * logn * (prod + red)):
        return (MATVEC, 0, 0, 0)
    if (n + n // 2) * nl * 4 <= 160 * 1024:
        return (LDS, 0, 0, lds_pb(n))
    if logn <= 22 and not stage_loop:
        l1 = (logn + 1) // 2
        return (FOUR_STEP, 1 << l1, 1 << (logn - l1), 0)
    return (STAGE_LOOP, 0, 0, 0)


def _partial_k(nl, n, d):
    """one k < n that still goes to the transform at this d: the largest below n / 2, else the smallest at or above it; where every
    partial k is a mat-vec, n / 2 - 1 (the mat-vec's partial output is checked then)"""
    on = [k for k in range(1, n) if route_model(nl, n, d, k)[0] != MATVEC]
    below = [k for k in on if k < n // 2]
    if below:
        return below[-1]
    if on:
        return on[0]
    return max(n // 2 - 1, 1) if n > 1 else 1


Case = collections.namedtuple("Case", "field n d k route")      # route: the whole answer of the query, (route, n1, n2, PB)


def _case(f, n, d, k, stage_loop=False):
    return Case(f.id, n, d, k, route_model(f.n_limbs, n, d, k, stage_loop))


# ---- (a) pruning sweep -----------------------------------------------------------------------------------------------------------
SWEEP_SMALL = [2, 4, 8, 16, 32, 64]
SWEEP_LARGE = [128, 256, 512, 1024, 2048]
SWEEP_LARGE_FIELDS = ["bls", "top", "gen-hi", "goldilocks", "tiny"]


def sweep_ds(n):
    if n <= 64:
        return list(range(1, n + 3))
    return [1, 2, 7, 8, 9, n // 8 - 1, n // 8, n // 8 + 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1, n, n + 5]


@functools.lru_cache(maxsize=None)
def sweep_cases(field_id, n):
    f = FIELD[field_id]
    out = []
    for d in sweep_ds(n):
        out.append(_case(f, n, d, n))
        if n > 1:
            out.append(_case(f, n, d, _partial_k(f.n_limbs, n, d)))
    return out


SWEEP = [(f.id, n) for n in SWEEP_SMALL for f in FIELDS] + [(fid, n) for n in SWEEP_LARGE for fid in SWEEP_LARGE_FIELDS]

# ragged last workgroup and the uidx % npoly lane map: (field, n, d), batches of PB - 1, PB, PB + 1, 2 PB + 3 polynomials
BATCH = [(fid, n, d) for fid in ("bls", "goldilocks") for n, d in ((2, 2), (8, 5), (64, 37), (2048, 1500))]


def batch_sizes(n):
    pb = lds_pb(n)
    return [c for c in (pb - 1, pb, pb + 1, 2 * pb + 3) if c > 0]


# ---- (b) lazy bound ----------------------------------------------------------------------------------------------------------------
LAZY_FIELDS = ["top", "psc-lo", "gen-hi", "w65", "tiny-wide", "n61"]
LAZY = [(fid, n) for fid in LAZY_FIELDS for n in (8, 64, 512, 2048)] + [("n61", 8192)]


def lazy_count(f, n):
    """rows a lazy-bound case: every pool value at every position for the orders where Python is quick"""
    return len(ev.edge_pool(f.p, f.n_limbs)) + 5 if n <= 64 else (8 if n == 512 else 6)


# ---- (c) four-step -----------------------------------------------------------------------------------------------------------------
FOUR_STEP_ORDERS = {"bls": [4096, 8192], "top": [4096, 8192], "gen-hi": [4096, 8192], "w65": [4096, 8192], "psc-lo": [4096], "stark": [4096],
                    "tiny-wide": [4096], "goldilocks": [1 << 14, 1 << 15], "n61": [1 << 14, 1 << 15]}
FOUR = [(fid, n) for fid, orders in FOUR_STEP_ORDERS.items() for n in orders]


def _smallest(pred, hi):
    return next(v for v in range(1, hi + 1) if pred(v))


@functools.lru_cache(maxsize=None)
def four_step_cases(field_id, n):
    """the calls of one (field, order) in the order they are made on one stream: k = n over the d list -- d = n first and the smallest d
    right behind it (a stale ntt4: scratch would show there) -- then d = n over the k list"""
    f = FIELD[field_id]
    route = route_model(f.n_limbs, n, n, n)
    assert route[0] == FOUR_STEP
    n1, n2 = route[1], route[2]
    dmin = _smallest(lambda d: route_model(f.n_limbs, n, d, n)[0] == FOUR_STEP, n)
    kmin = _smallest(lambda k: route_model(f.n_limbs, n, n, k)[0] == FOUR_STEP, n)
    ds = [n, dmin, n2 - 1, n2, n2 + 1, n, 2 * n2 + 1, n - 1, n + 7]
    ks = [kmin, n1 - 1, n1, n1 + 1, n - 1]
    return [_case(f, n, d, n) for d in ds] + [_case(f, n, n, k) for k in ks]


@functools.lru_cache(maxsize=None)
def stage_loop_cases(field_id):
    """one d and one k a field at its smallest four-step order, under HB_NTT_STAGE_LOOP=1"""
    f = FIELD[field_id]
    n = FOUR_STEP_ORDERS[field_id][0]
    n1, n2 = route_model(f.n_limbs, n, n, n)[1:3]
    return [_case(f, n, 2 * n2 + 1, n, stage_loop=True), _case(f, n, n, n1 + 1, stage_loop=True)]


# ---- (d) twiddle tables keyed by the root: (field, order, d) at an LDS and at a four-step order ------------------------------------------
ROOTS = [("bls", 64, 64), ("bls", 4096, 4096), ("goldilocks", 64, 64), ("goldilocks", 1 << 14, 1 << 14), ("gen-hi", 512, 300)]

# ---- (f) interpolation at omega^zs ---------------------------------------------------------------------------------------------------
INTERP_FIELDS = ["gen-hi", "w65", "n61", "tiny"]
INTERP_ORDER = 32
INTERP_KS = [1, 2, 16, 17, 32]
INTERP_BATCHES = [1, 70]


def interp_values(p, k, count, seed):
    """half pool values, half uniform ones"""
    pool = ev.edge_pool(p, ev.n_limbs_of(p))
    rnd = random.Random(seed)
    return [[rnd.choice(pool) if rnd.random() < 0.5 else rnd.randrange(p) for _ in range(k)] for _ in range(count)]


def all_transform_cases():
    """every Case of the lists above (the batch, lazy and root lists as the k = n cases they run)"""
    out = []
    for fid, n in SWEEP:
        out += sweep_cases(fid, n)
    out += [_case(FIELD[fid], n, d, n) for fid, n, d in BATCH]
    out += [_case(FIELD[fid], n, n, n) for fid, n in LAZY]
    for fid, n in FOUR:
        out += four_step_cases(fid, n)
    for fid in FOUR_STEP_ORDERS:
        out += stage_loop_cases(fid)
    out += [_case(FIELD[fid], n, d, n) for fid, n, d in ROOTS]
    return out
