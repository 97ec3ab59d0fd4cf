"""
Offline-phase encodes on device tensors: the same kernels as the batch open, large
batches, no new arithmetic.

* ShareDealer       -- the trusted dealer's share generation: k polynomials of degree t evaluated at the n
                       party points, party-major so that row i is party i's file
                       (reference preprocessing.py:211-239 `_write_polys`; offline_randousha.py:41-53).
* HyperInvertible   -- RanDouSha's refinement: the n parties' contributions are the coefficients of a
                       degree n-1 polynomial, evaluated at the n party points
                       (reference offline_randousha.py:73-78), and the checkers' degree / secret test
                       (reference :95-123).
* random_elements   -- uniform field elements drawn on the device (rejection from 2^bits).

* extract_at_omega_powers -- the randomness extractor of progs/random_refinement.py for any number of contribution vectors.

The protocol that makes preprocessing among the parties (reference offline_randousha.py; csrc/hb_off.hip):

* randousha         -- (n - 2t) k pairs (r_t, r_2t) of sharings of random values nobody knows (:34-151)
* generate_triples  -- k Beaver triples by degree reduction (:154-191)
* generate_bits     -- k shared random bits, as +-1 or as 0 / 1 (:194-232)
* generate_matrix_triples -- matrix triples (P, Q, P Q) for linalg.beaver_matmul: generate_triples with a matrix product in the middle
* generate_powers   -- shares of b, b^2, .., b^k of random b, by doubling: ceil(log2 k) opens (csrc/hb_offpow.hip; not in the reference)
* generate_cubes    -- shares of (r, r^2, r^3) for MiMC's rounds: the same chain with k = 3, two opens
* mul_add, invsqrt_scale, degree_check -- the three kernels on tensors; invsqrt_model, degree_check_model -- on Python ints
* pow_mask, pow_finish -- the two launches of a doubling level on tensors; power_levels, powers_model -- the levels, and on Python ints
* generate_share_bits -- random residues shared together with their bit planes (the reference's get_share_bits, which it deals), by
                       rejection of bitwise-shared candidates: bits, triples, one carry tree and one open a round (csrc/hb_offsb.hip)
* generate_less_than_preprocessing -- (r, r_bits, triples, s, s_bits) as share_comparison.less_than takes them, no dealer
* share_bits_round  -- one round over given bit planes and triples -> (r, r_bits, verdicts)
* sb_leaves, sb_finish -- the two launches of a round on tensors; share_bits_model, share_bits_candidates -- a candidate on Python ints,
                       and the number of candidates a round draws

Element layout as in honeybadgermpc_amd.device: int64 tensors (count, 4), little-endian limbs.
"""
import asyncio
import collections
import ctypes

import numpy as np

from . import wire
from ._capi import HB_LT_DIRECT, HB_OFF_01, HB_OFF_PM1, Context, HbView, np_ptr
from .device import BatchOpen
from .exceptions import HoneyBadgerMPCError

PM1, ZERO_ONE = HB_OFF_PM1, HB_OFF_01            # generate_bits' encodings: a share of +-1 (the reference's) or of 0 / 1


def random_elements(modulus, count, generator=None, device=None):
    """count uniform residues mod `modulus` as a (count, 4) limb tensor: bits-wide draws, rejected when >= modulus."""
    ctx = Context.get(modulus, device)
    t = ctx.torch
    bits = modulus.bit_length()
    top = (bits - 1) // 64                    # highest limb in use
    top_mask = (1 << (bits - 64 * top)) - 1
    nl = ctx.n_limbs
    p_limbs = [(modulus >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(nl)]
    sign = 1 << 63

    def as_i64(v):                            # the int64 with the same bits
        return v - (1 << 64) if v >= sign else v

    out, have = [], 0
    while have < count:
        want = max(1024, int((count - have) * 1.3) + 16)
        cand = t.randint(-(1 << 63), (1 << 63) - 1, (want, nl), dtype=t.int64, device=ctx.tdev, generator=generator)
        cand[:, top] &= as_i64(top_mask)
        for j in range(top + 1, nl):
            cand[:, j] = 0
        # unsigned lexicographic cand < p from the top limb down (x ^ sign turns unsigned order into signed order)
        less = t.zeros(want, dtype=t.bool, device=ctx.tdev)
        equal = t.ones(want, dtype=t.bool, device=ctx.tdev)
        for j in range(nl - 1, -1, -1):
            cj = cand[:, j] ^ as_i64(sign)
            pj = as_i64(p_limbs[j] ^ sign)
            less |= equal & (cj < pj)
            equal &= cj == pj
        keep = cand[less]
        out.append(keep[: count - have])
        have += out[-1].shape[0]
    return t.cat(out, dim=0).contiguous()


class ShareDealer:
    """deal(coeffs): [k][degree+1] coefficient rows (flat (k (degree+1), 4) tensor) -> [n][k] shares, row i = party i.

    It is the R1 encode of the batch open: the matrix-core path when the shape qualifies."""

    def __init__(self, modulus, n, t, max_polys=1 << 16, device=None, degree=None):
        """degree: of the dealt polynomials (default t; RanDouSha also deals at 2 t)"""
        self.n, self.t, self.d = n, t, (t if degree is None else degree) + 1
        self.op = BatchOpen(modulus, n, t, degree=degree, max_shares=max_polys * self.d, device=device)
        self.ctx = self.op.ctx

    def deal(self, coeffs, out=None):
        assert coeffs.shape[0] % self.d == 0
        return self.op.r1_encode(coeffs, out=out)

    def deal_secrets(self, secrets, generator=None):
        """Random polynomials of the dealer's degree with the given constant terms (a (k, 4) tensor) -> ([n][k] shares, coeffs)."""
        k = secrets.shape[0]
        coeffs = random_elements(self.ctx.modulus, k * self.d, generator, self.ctx.device).view(k, self.d, self.ctx.n_limbs)
        coeffs[:, 0, :] = secrets
        coeffs = coeffs.reshape(k * self.d, self.ctx.n_limbs).contiguous()
        return self.deal(coeffs), coeffs


class HyperInvertible:
    """RanDouSha's two codec steps for one party, k values per party.

    refine(received):  received[s][j] = the share sender s dealt us for its j-th value  ([n][k], party-major)
                       -> [n][k]: row i = the refined sharing i of every column, i.e. the polynomial with
                       coefficients received[0..n-1][j] evaluated at point(i).
    check(shares, degree): shares[s][j] = party s's share of checked value j ([n][k]) -> (ok, secrets):
                       every interpolated polynomial has exactly the given degree; secrets = constant terms.
    """

    def __init__(self, modulus, n, device=None):
        from .field import GF
        from .polynomial import EvalPoint

        self.ctx = ctx = Context.get(modulus, device)
        self.n = n
        point = EvalPoint(GF(modulus), n, use_omega_powers=False)
        self.x = [point(i).value for i in range(n)]
        self._xh = ctx.host_elems(self.x)
        m = ctypes.c_void_p()
        ctx.check(ctx.lib.hb_vand_matrix_create(ctx.h, np_ptr(self._xh), n, n, ctypes.byref(m), ctx.stream()), "hb_vand_matrix_create")
        self._v = m

    def refine(self, received, out=None):
        received = self.ctx.elems(received, what="received")
        n, k = self.n, received.shape[0] // self.n
        if received.shape[0] != n * k:
            raise ValueError("received: expected n rows of k elements")
        if out is None:
            out = self.ctx.empty(n * k)
        view = HbView(1, k)                   # element (column j, row l) at l * k + j, for the input and the output
        rc = self.ctx.lib.hb_matvec(self.ctx.h, self._v, self.ctx.ptr(received), view, None, self.ctx.ptr(out), view, k, self.ctx.stream())
        self.ctx.check(rc, "hb_matvec")
        return out

    def check(self, shares, degree):
        shares = self.ctx.elems(shares, what="shares")
        t = self.ctx.torch
        n, k = self.n, shares.shape[0] // self.n
        rows = shares.view(n, k, self.ctx.n_limbs).transpose(0, 1).contiguous().view(k * n, self.ctx.n_limbs)     # [k][n]: one polynomial's points per row
        coeffs = self.ctx.empty(k * n)
        rc = self.ctx.lib.hb_vandermonde_batch_interpolate(self.ctx.h, np_ptr(self._xh), n, self.ctx.ptr(rows), k, self.ctx.ptr(coeffs), self.ctx.stream())
        self.ctx.check(rc, "hb_vandermonde_batch_interpolate")
        nz = (coeffs.view(k, n, self.ctx.n_limbs) != 0).any(dim=2)                                 # [k][n] coefficient is non-zero
        ok = bool(nz[:, degree].all().item()) and not bool(nz[:, degree + 1 :].any().item())
        return ok, coeffs.view(k, n, self.ctx.n_limbs)[:, 0, :].contiguous()

    def __del__(self):
        try:
            self.ctx.lib.hb_matrix_destroy(self._v)
        except Exception:
            pass


def extract_at_omega_powers(field, n, t, batches):
    """Randomness extraction (reference progs/random_refinement.py:5-19) for a list of contribution vectors.

    Each vector holds k contributions (n - t <= k <= n, n >= 3 t + 1), read as the coefficients of a polynomial; the result
    keeps its values at the first k - t omega points.  All vectors of one length go through ONE batched encode."""
    from .polynomial import EvalPoint
    from .reed_solomon import EncoderFactory

    if n < 3 * t + 1:
        raise AssertionError(f"randomness extraction needs n >= 3 t + 1 (n = {n}, t = {t})")
    for vec in batches:
        if not n - t <= len(vec) <= n:
            raise AssertionError(f"randomness extraction: {len(vec)} contributions with n = {n}, t = {t}")
    codec = EncoderFactory.get(EvalPoint(field, n, use_omega_powers=True))
    out = [None] * len(batches)
    for k in sorted({len(vec) for vec in batches}):
        which = [i for i, vec in enumerate(batches) if len(vec) == k]
        for i, row in zip(which, codec.encode([list(batches[i]) for i in which])):
            out[i] = row[: k - t]
    return out


# ---- the offline phase among the parties (reference offline_randousha.py) --------------------------------------------------------
def _tonelli_constants(p):
    """p - 1 = q 2^s and c = z^q for the smallest non-residue z >= 2 (csrc/hb_sqrt.hip's choice) -> (q, s, c)"""
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    return q, s, pow(z, q, p)


def invsqrt_model(x, p):
    """x^(-1/2) mod p on Python ints as hb_off_invsqrt_scale defines it: w = x^((q-1)/2) c^e with the unique e in [0, 2^(s-1))
    for which x^q c^(2e) = 1 -> (w, status); status 0, or 1 for x = 0 and 2 for a non-residue (w = 0 for both)."""
    x %= p
    if x == 0:
        return 0, 1
    q, s, c = _tonelli_constants(p)
    t = pow(x, q, p)
    if pow(t, 1 << (s - 1), p) != 1:              # the order of x^q is the full 2^s: no even power of c cancels it
        return 0, 2
    e = 0
    for i in range(s - 1):                        # bit i of e: t c^(2 e_low) has order dividing 2^(s-1-i); is it 2^(s-1-i) itself?
        if pow(t * pow(c, 2 * e, p) % p, 1 << (s - 2 - i), p) != 1:
            e |= 1 << i
    assert t * pow(c, 2 * e, p) % p == 1
    return pow(x, (q - 1) // 2, p) * pow(c, e, p) % p, 0


def degree_check_model(coeffs, n, k, t):
    """hb_off_degree_check on Python ints: coeffs [n][2k] flat, coefficient-major -> [not of exact degree t, not of exact degree 2t,
    constants differ], counts over the k columns"""
    bad = [0, 0, 0]
    for j in range(k):
        for which, (col, deg) in enumerate(((j, t), (k + j, 2 * t))):
            poly = [coeffs[e * 2 * k + col] for e in range(n)]
            bad[which] += poly[deg] == 0 or any(poly[deg + 1:])
        bad[2] += coeffs[j] != coeffs[k + j]
    return bad


def _out_like(ctx, out, like, count):
    if out is None:
        return ctx.torch.empty_like(like)
    if isinstance(out, ctx.torch.Tensor) and not out.is_contiguous():
        raise ValueError("out: must be contiguous")
    return ctx.elems(out, count, what="out")


def mul_add(ctx, a, b, c, out=None):
    """a b + c element by element in one launch (three reads, one write).  b may be a, and out may be any of the inputs."""
    a = ctx.elems(a, what="a")
    count = a.numel() // ctx.n_limbs
    b, c = ctx.elems(b, count, what="b"), ctx.elems(c, count, what="c")
    out = _out_like(ctx, out, a, count)
    ctx.check(ctx.lib.hb_off_mul_add(ctx.h, ctx.ptr(a), ctx.ptr(b), ctx.ptr(c), ctx.ptr(out), count, ctx.stream()), "hb_off_mul_add")
    return out


def invsqrt_scale(ctx, x, u=None, mode=PM1, check=True, out=None):
    """w = x^(-1/2) (invsqrt_model) of every public x, scaled onto the shares u: mode PM1 -> u w, ZERO_ONE -> (u w + 1) / 2; u None -> w.
    check=True reads the two status words back -- one synchronisation -- and raises AssertionError when an x was zero or a
    non-residue, as the reference's GFElement.sqrt does for both.  check=False -> (out, status): an int32 tensor [zeros,
    non-residues] once the stream has got there; their outputs are 0 and the others are right either way.  Nothing synchronises."""
    if mode not in (PM1, ZERO_ONE) or isinstance(mode, bool):
        raise ValueError("mode: PM1 or ZERO_ONE")
    x = ctx.elems(x, what="x")
    count = x.numel() // ctx.n_limbs
    if u is not None:
        u = ctx.elems(u, count, what="u")
    out = _out_like(ctx, out, x, count)
    status = ctx.torch.zeros(2, dtype=ctx.torch.int32, device=ctx.tdev)
    rc = ctx.lib.hb_off_invsqrt_scale(ctx.h, ctx.ptr(x), None if u is None else ctx.ptr(u), mode, ctx.ptr(out), count, ctx.ptr(status), ctx.stream())
    ctx.check(rc, "hb_off_invsqrt_scale")
    if not check:
        return out, status
    zeros, nonres = (int(v) for v in status.tolist())
    if zeros or nonres:
        raise AssertionError(f"no square root: {zeros} zeros and {nonres} non-residues among {count} values")
    return out


def degree_check(ctx, coeffs, n, t, check=True):
    """The checkers' verdict on a coefficient-major [n][2k] block (degree_check_model).  check=True -> the three counts as ints (one
    synchronisation); check=False -> the int32[3] tensor, nothing synchronises."""
    coeffs = ctx.elems(coeffs, what="coeffs")
    rows = coeffs.numel() // ctx.n_limbs
    if n < 1 or t < 0 or 2 * t >= n or rows % (2 * n):
        raise ValueError("coeffs: expected n rows of 2 k elements, 2 t < n")
    counters = ctx.torch.zeros(3, dtype=ctx.torch.int32, device=ctx.tdev)
    rc = ctx.lib.hb_off_degree_check(ctx.h, ctx.ptr(coeffs), n, rows // (2 * n), t, ctx.ptr(counters), ctx.stream())
    ctx.check(rc, "hb_off_degree_check")
    return tuple(int(v) for v in counters.tolist()) if check else counters


class _Codec:
    """what one party's RanDouSha needs per (field, n, t): the two dealers, the refinement and the inverse Vandermonde matrix"""

    _cache = {}

    @classmethod
    def get(cls, ctx, n, t, k):
        cap = 1 << max(10, (k - 1).bit_length())
        key = (ctx.modulus, ctx.device, n, t)
        self = cls._cache.get(key)
        if self is None or self.cap < cap:
            self = cls._cache[key] = cls(ctx, n, t, cap)
        return self

    def __init__(self, ctx, n, t, cap):
        self.ctx, self.n, self.t, self.cap = ctx, n, t, cap
        self.deal_t = ShareDealer(ctx.modulus, n, t, max_polys=cap, device=ctx.device)
        self.deal_2t = ShareDealer(ctx.modulus, n, t, max_polys=cap, device=ctx.device, degree=2 * t)
        self.hyper = HyperInvertible(ctx.modulus, n, device=ctx.device)
        m = ctypes.c_void_p()
        ctx.check(ctx.lib.hb_vand_inverse_create(ctx.h, np_ptr(self.hyper._xh), n, ctypes.byref(m), ctx.stream()), "hb_vand_inverse_create")
        self._vinv = m

    def interpolate(self, block, width):
        """[n][width] values at the party points -> [n][width] coefficients, coefficient-major: one mat-vec, no transpose"""
        out = self.ctx.empty(self.n * width)
        view = HbView(1, width)
        rc = self.ctx.lib.hb_matvec(self.ctx.h, self._vinv, self.ctx.ptr(block), view, None, self.ctx.ptr(out), view, width, self.ctx.stream())
        self.ctx.check(rc, "hb_matvec")
        return out

    def __del__(self):
        try:
            self.ctx.lib.hb_matrix_destroy(self._vinv)
        except Exception:
            pass


_SUCCESS, _ABORT = "S", "A"                       # HyperInvMessageType
_INCONSISTENT = "Aborting because the shares were inconsistent."


class _Verdicts:
    """The H3 channel of one run, read from the start: a party still waiting for shares learns of an abort (a checker's, or a party's
    that met a malformed message) instead of waiting for a message that will not come."""

    def __init__(self, recv):
        self.received, self.aborted = [], asyncio.Event()
        self._more = asyncio.Event()
        self._task = asyncio.ensure_future(self._pump(recv))

    async def _pump(self, recv):
        while True:
            sender, msg = await recv()
            self.received.append((sender, msg))
            if msg != _SUCCESS:
                self.aborted.set()
            self._more.set()

    async def guard(self, coro):
        """await coro, unless an abort arrives first"""
        work, stop = asyncio.ensure_future(coro), asyncio.ensure_future(self.aborted.wait())
        try:
            await asyncio.wait({work, stop}, return_when=asyncio.FIRST_COMPLETED)
            if not work.done():
                raise HoneyBadgerMPCError(_INCONSISTENT)
            return work.result()
        finally:
            work.cancel()
            stop.cancel()

    async def successes(self, checkers):
        """wait for a verdict of every checker -> True when all are successes"""
        while not self.aborted.is_set() and len({s for s, _ in self.received if s in checkers}) < len(checkers):
            self._more.clear()
            await self._more.wait()
        return not self.aborted.is_set()

    def close(self):
        self._task.cancel()


async def _recv_rows(ctx, recv, n, width):
    """one (width, limbs) blob from every party -> host array [n][width][limbs]; anything else raises HoneyBadgerMPCError"""
    rows = np.zeros((n, width, ctx.n_limbs), dtype=np.uint64)
    seen = set()
    while len(seen) < n:
        sender, blob = await recv()
        try:
            a = wire.unpack_limbs(blob)
        except ValueError as e:
            raise HoneyBadgerMPCError(f"malformed share message from party {sender}: {e}") from None
        if a.shape != (width, ctx.n_limbs) or not isinstance(sender, int) or not 0 <= sender < n or sender in seen:
            raise HoneyBadgerMPCError(f"malformed share message from party {sender}")
        rows[sender] = a
        seen.add(sender)
    return rows


async def randousha(co, k, tag="randousha", generator=None):
    """(n - 2t) k pairs of sharings (r_t, r_2t) of the same random values, of degree t and 2t (reference offline_randousha.py:34-151,
    step by step): every party draws k secrets and deals each at both degrees, one blob row_t[i] || row_2t[i] to party i (H1); the
    received [n][2k] block is refined by one hyper-invertible mat-vec; refined rows n - 2t .. n - 1 go to their checkers (H2), who
    interpolate with one inverse mat-vec, judge degrees and constants in one launch (hb_off_degree_check) and tell everyone "S" or
    "A" (H3).  Anything but 2t successes -- and a malformed message, of which the others are told by an "A" -- raises
    HoneyBadgerMPCError.  Waits for all n parties, as the reference does.
    -> (r_t, r_2t), ((n - 2t) k, limbs) each; element j (n - 2t) + i is refined sharing i of column j (the reference's order).
    co: an OpenCoalescer (n, t, myid, ctx, get_send_recv); channels are (tag, "H1"), (tag, "H2"), (tag, "H3")."""
    n, t, me, ctx = co.n, co.t, co.myid, co.ctx
    if not (isinstance(k, int) and k >= 1 and t >= 1 and n >= 3 * t + 1):
        raise ValueError("randousha: t >= 1, n >= 3 t + 1 and k >= 1")
    torch, L = ctx.torch, ctx.n_limbs
    codec = _Codec.get(ctx, n, t, k)
    good = n - 2 * t
    checkers = set(range(good, n))
    send1, recv1 = co.get_send_recv((tag, "H1"))
    send2, recv2 = co.get_send_recv((tag, "H2"))
    send3, recv3 = co.get_send_recv((tag, "H3"))
    verdicts = _Verdicts(recv3)

    def rows_out(block, send, to):
        host = block.view(n, 2 * k, L).cpu().numpy().view(np.uint64)          # one copy for every recipient's row
        for i in to:
            send(i, wire.pack_limbs(host[i]))

    async def rows_in(recv):
        try:
            host = await verdicts.guard(_recv_rows(ctx, recv, n, 2 * k))
        except HoneyBadgerMPCError:
            for i in range(n):
                send3(i, _ABORT)
            raise
        return ctx.reduce_(ctx.to_device(host.reshape(n * 2 * k, L)))         # from outside: residues count

    try:
        secrets = random_elements(ctx.modulus, k, generator, ctx.device)
        unref_t, _ = codec.deal_t.deal_secrets(secrets, generator)
        unref_2t, _ = codec.deal_2t.deal_secrets(secrets, generator)
        rows_out(torch.cat((unref_t.view(n, k, L), unref_2t.view(n, k, L)), dim=1).contiguous(), send1, range(n))
        refined = codec.hyper.refine(await rows_in(recv1))                     # [n][2k]: row i = refined sharing i of every column
        rows_out(refined, send2, sorted(checkers))
        if me in checkers:
            bad = degree_check(ctx, codec.interpolate(await rows_in(recv2), 2 * k), n, t)
            for i in range(n):
                send3(i, _ABORT if any(bad) else _SUCCESS)
        if not await verdicts.successes(checkers):
            raise HoneyBadgerMPCError(_INCONSISTENT)
    finally:
        verdicts.close()
    kept = refined.view(n, 2 * k, L)[:good]
    return (kept[:, :k].transpose(0, 1).reshape(good * k, L).contiguous(), kept[:, k:].transpose(0, 1).reshape(good * k, L).contiguous())


async def generate_triples(co, k, tag="triples", generator=None):
    """k Beaver triples (a, b, ab), (k, limbs) each, by degree reduction (reference offline_randousha.py:154-191): a, b and a mask r
    from RanDouSha, ab = open(a b + r_2t, degree 2t) - r_t -- one fused launch (hb_off_mul_add), one coalesced open, one sub.
    One deliberate difference: the reference runs randousha(3k) and uses 3k of the (n - 2t) 3k sharings it made; this runs
    randousha(ceil(3k / (n - 2t))) and slices.  The outputs are random sharings either way."""
    from .share_arithmetic import sub

    if not (isinstance(k, int) and k >= 1):
        raise ValueError("generate_triples: k >= 1")
    ctx, good = co.ctx, co.n - 2 * co.t
    r_t, r_2t = await randousha(co, -(-3 * k // good), tag=(tag, "randousha"), generator=generator)
    a, b, r = (r_t[i * k:(i + 1) * k] for i in range(3))
    opened = await co.open_share_array(mul_add(ctx, a, b, r_2t[2 * k:3 * k]), degree=2 * co.t)
    return a.clone(), b.clone(), sub(ctx, opened, r)


async def generate_matrix_triples(co, m, k, n, count=1, tag="matrix_triples", generator=None):
    """count matrix triples (P, Q, PQ = P Q), P (count, m, k, limbs), Q (count, k, n, limbs), PQ (count, m, n, limbs), by degree
    reduction -- the matrix form of generate_triples: P, Q and a mask r come from ONE randousha, and
    PQ = open(P Q + r_2t, degree 2t) - r_t: one launch (linalg.matmul with the mask as its epilogue), one coalesced open of
    count m n elements, one sub.  The same slicing and the same abort behaviour as generate_triples, because it only composes
    randousha: anything but 2t successes raises HoneyBadgerMPCError in every party."""
    from .linalg import matmul
    from .share_arithmetic import sub

    for v, what in ((m, "m"), (k, "k"), (n, "n"), (count, "count")):
        if not (isinstance(v, int) and not isinstance(v, bool) and v >= 1):
            raise ValueError(f"generate_matrix_triples: {what} >= 1")
    ctx, good, L = co.ctx, co.n - 2 * co.t, co.ctx.n_limbs
    np_, nq, nr = count * m * k, count * k * n, count * m * n
    r_t, r_2t = await randousha(co, -(-(np_ + nq + nr) // good), tag=(tag, "randousha"), generator=generator)
    P = r_t[:np_].clone().view(count, m, k, L)
    Q = r_t[np_:np_ + nq].clone().view(count, k, n, L)
    r = r_t[np_ + nq:np_ + nq + nr]
    masked = matmul(ctx, P, Q, add=r_2t[np_ + nq:np_ + nq + nr])
    opened = await co.open_share_array(masked.view(nr, L), degree=2 * co.t)
    return P, Q, sub(ctx, opened, r).view(count, m, n, L)


async def generate_bits(co, k, encoding=PM1, tag="bits", generator=None):
    """k shared random bits, (k, limbs) (reference offline_randousha.py:194-232): u and a mask r from RanDouSha,
    u^2 = open(open(u u + r_2t, degree 2t) - r_t), and u / sqrt(u^2) by the fused inverse root (hb_off_invsqrt_scale): two coalesced
    opens in all.  encoding PM1 -> shares of +-1 (the reference's), ZERO_ONE -> of 0 / 1, the bit planes fixedpoint and
    share_comparison take.  An opened u^2 that is zero (probability 1 / p) or a non-residue raises AssertionError, as the
    reference's sqrt does."""
    from .share_arithmetic import sub

    if not (isinstance(k, int) and k >= 1):
        raise ValueError("generate_bits: k >= 1")
    if encoding not in (PM1, ZERO_ONE) or isinstance(encoding, bool):
        raise ValueError("encoding: PM1 or ZERO_ONE")
    ctx, good = co.ctx, co.n - 2 * co.t
    r_t, r_2t = await randousha(co, -(-2 * k // good), tag=(tag, "randousha"), generator=generator)
    u, r = r_t[:k], r_t[k:2 * k]
    opened = await co.open_share_array(mul_add(ctx, u, u, r_2t[k:2 * k]), degree=2 * co.t)
    squares = await co.open_share_array(sub(ctx, opened, r, out=opened))
    return invsqrt_scale(ctx, squares, u, encoding, check=True)


# ---- shared powers and cubes (csrc/hb_offpow.hip; the reference deals both, preprocessing.py) --------------------------------------
def power_levels(k):
    """The doubling levels that grow b^1 into b^1 .. b^k: a list of (m, w), w = min(m, k - m).  With powers 1 .. m held, level (m, w)
    makes b^(m+1+j) = b^m b^(j+1) for j < w.  ceil(log2 k) levels, k - 1 products; k = 1 -> []."""
    if not (isinstance(k, int) and not isinstance(k, bool) and k >= 1):
        raise ValueError("power_levels: k >= 1")
    levels, m = [], 1
    while m < k:
        w = min(m, k - m)
        levels.append((m, w))
        m += w
    return levels


def powers_model(b, k, p):
    """[b^1 .. b^k] mod p on Python ints, by the products the levels make"""
    out = [b % p]
    for m, w in power_levels(k):
        out += [out[m - 1] * out[j] % p for j in range(w)]
    return out


_LAYOUTS = ("item", "power")


def _pow_operands(ctx, powers, m, w, layout):
    """-> (count, k, item_stride, power_stride) of a contiguous (count, k, limbs) ("item") or (k, count, limbs) ("power") tensor"""
    if layout not in _LAYOUTS:
        raise ValueError(f"layout: one of {_LAYOUTS}, got {layout!r}")
    if not isinstance(powers, ctx.torch.Tensor) or powers.dim() != 3:
        raise ValueError(f"powers: expected a tensor of shape (count, k, {ctx.n_limbs}) or (k, count, {ctx.n_limbs})")
    if not powers.is_contiguous():
        raise ValueError("powers: must be contiguous")
    ctx.elems(powers, what="powers")
    count, k = (int(powers.shape[0]), int(powers.shape[1])) if layout == "item" else (int(powers.shape[1]), int(powers.shape[0]))
    for v in (m, w):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError("m, w: integers")
    if not (1 <= w <= m and m + w <= k):
        raise ValueError(f"level ({m}, {w}): 1 <= w <= m and m + w <= k = {k}")
    return (count, k, k, 1) if layout == "item" else (count, k, 1, count)


def pow_mask(ctx, powers, r2t, m, w, layout="item", out=None):
    """One level's masked products in one launch: out[c w + j] = P[c][m] P[c][j+1] + r2t[c w + j], (count w, limbs), contiguous.
    powers: (count, k, limbs) for layout "item", (k, count, limbs) for "power"; it is only read."""
    count, _, item_stride, power_stride = _pow_operands(ctx, powers, m, w, layout)
    r2t = ctx.elems(r2t, count * w, what="r2t")
    out = ctx.empty(count * w) if out is None else _out_like(ctx, out, r2t, count * w)
    rc = ctx.lib.hb_off_pow_mask(ctx.h, ctx.ptr(powers), item_stride, power_stride, ctx.ptr(r2t), m, w, ctx.ptr(out), count, ctx.stream())
    ctx.check(rc, "hb_off_pow_mask")
    return out


def pow_finish(ctx, opened, rt, powers, m, w, layout="item"):
    """One level's finish in one launch: P[c][m+1+j] = opened[c w + j] - rt[c w + j], written into `powers` in place (columns m .. m+w-1
    alone) -> powers."""
    count, _, item_stride, power_stride = _pow_operands(ctx, powers, m, w, layout)
    opened, rt = ctx.elems(opened, count * w, what="opened"), ctx.elems(rt, count * w, what="rt")
    rc = ctx.lib.hb_off_pow_finish(ctx.h, ctx.ptr(opened), ctx.ptr(rt), ctx.ptr(powers), item_stride, power_stride, m, w, count, ctx.stream())
    ctx.check(rc, "hb_off_pow_finish")
    return powers


def _positive_int(v, what):
    if not (isinstance(v, int) and not isinstance(v, bool) and v >= 1):
        raise ValueError(f"{what} >= 1")


async def _powers(co, count, k, tag, generator, layout):
    """the chain of generate_powers over `count` items -> the (count, k, limbs) or (k, count, limbs) tensor"""
    ctx, good, L = co.ctx, co.n - 2 * co.t, co.ctx.n_limbs
    r_t, r_2t = await randousha(co, -(-count * k // good), tag=(tag, "randousha"), generator=generator)
    torch = ctx.torch
    powers = torch.empty((count, k, L) if layout == "item" else (k, count, L), dtype=torch.int64, device=ctx.tdev)
    (powers[:, 0] if layout == "item" else powers[0]).copy_(r_t[:count])
    levels = power_levels(k)
    masked = ctx.empty(count * max((w for _, w in levels), default=0))       # an open is over before the next level writes here
    at = count
    for m, w in levels:
        size = count * w
        pow_mask(ctx, powers, r_2t[at:at + size], m, w, layout, out=masked[:size])
        opened = await co.open_share_array(masked[:size], degree=2 * co.t)
        pow_finish(ctx, opened, r_t[at:at + size], powers, m, w, layout)
        at += size
    return powers


async def generate_powers(co, count, k, tag="powers", generator=None, layout="item"):
    """Shares of b_c, b_c^2, .., b_c^k for `count` random b_c nobody knows: (count, k, limbs) for layout "item" (what
    power_mixing.power_mix and solver.mix take), (k, count, limbs) for "power".  One randousha(ceil(count k / (n - 2t))) supplies the
    b (its first count t-sharings) and a mask pair (r_t, r_2t) for each of the count (k - 1) products; the powers grow by doubling
    (power_levels): a level is one launch that masks b^m b^(j+1) + r_2t for every item and j, ONE coalesced open at degree 2t, and one
    launch that writes opened - r_t into the powers array in place -- ceil(log2 k) opens in all, none for k = 1.  Aborts are
    randousha's: anything but 2t successes raises HoneyBadgerMPCError in every party."""
    _positive_int(count, "generate_powers: count")
    _positive_int(k, "generate_powers: k")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout: one of {_LAYOUTS}, got {layout!r}")
    return await _powers(co, count, k, tag, generator, layout)


async def generate_cubes(co, rounds, count, tag="cubes", generator=None):
    """(r, r2, r3), (rounds, count, limbs) each: shares of random r, r^2, r^3, what progs.mimc.mimc_mpc_batch and mimc_decrypt take.
    The chain of generate_powers with k = 3 over rounds count items in the power-major layout: two opens, and the three results are
    views of one (3, rounds count, limbs) buffer -- nothing is transposed."""
    _positive_int(rounds, "generate_cubes: rounds")
    _positive_int(count, "generate_cubes: count")
    powers = await _powers(co, rounds * count, 3, tag, generator, "power")
    return tuple(powers[e].view(rounds, count, co.ctx.n_limbs) for e in range(3))


# ---- share bits: a random residue with its bit planes (csrc/hb_offsb.hip; the reference deals them, preprocessing.py get_share_bits) --
def share_bits_model(bits, p):
    """One candidate on Python ints: bits b_0 .. b_{L-1}, least significant first, L = bit_length(p) -> (r, accepted) with
    r = sum_i 2^i b_i, an integer below 2^L, and accepted = r < p.  A kept r is uniform in [0, p) when the bits are uniform."""
    L = p.bit_length()
    bits = list(bits)
    if len(bits) != L or any(b not in (0, 1) or isinstance(b, bool) for b in bits):
        raise ValueError(f"bits: expected {L} values 0 or 1")
    r = sum(b << i for i, b in enumerate(bits))
    return r, r < p


def share_bits_candidates(p, count):
    """The number m of candidates one round draws for `count` residues.  With a = p / 2^L the number kept among m candidates is
    binomial, of mean m a and variance m a (1 - a); m is the smallest number whose mean lies four standard deviations above the
    count: m a - 4 sqrt(m a (1 - a)) > count - 1.  The number kept is an integer, so a lower bound above count - 1 is a lower bound
    of count -- with ">= count" instead, a field like 2^64 - 59, where a candidate is rejected with probability 2^-58, would ask for
    one spare candidate whatever the count.  Evaluated on integers (X = m p - (count - 1) 2^L > 0 and X^2 > 16 m p (2^L - p)), so
    every party gets the same m.  A round that keeps fewer is followed by another: m decides cost, never correctness."""
    if not (isinstance(p, int) and not isinstance(p, bool) and p >= 3):
        raise ValueError("share_bits_candidates: p >= 3")
    if not (isinstance(count, int) and not isinstance(count, bool) and count >= 0):
        raise ValueError("share_bits_candidates: count >= 0")
    if count == 0:
        return 0
    N = 1 << p.bit_length()

    def enough(m):
        x = m * p - (count - 1) * N
        return x > 0 and x * x > 16 * m * p * (N - p)

    lo, hi = count - 1, count                     # enough(lo) is false: m a < m; the left side grows with m once it is positive
    while not enough(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if enough(mid) else (mid, hi)
    return hi


def _sb_planes(ctx, bits):
    """the candidates' bit planes: a contiguous (L, m, limbs) tensor -> (bits, L, m)"""
    L = ctx.modulus.bit_length()
    if not isinstance(bits, ctx.torch.Tensor) or bits.dim() != 3 or bits.shape[0] != L:
        raise ValueError(f"bits: expected a tensor of shape ({L}, count, {ctx.n_limbs})")
    if not bits.is_contiguous():
        raise ValueError("bits: must be contiguous")
    return ctx.elems(bits, what="bits"), L, int(bits.shape[1])


def sb_leaves(ctx, bits, bound=None):
    """-> (g, p), (L, count, limbs) each: the leaves of the carry tree for [r > bound] over candidates given as bit planes
    (L, count, limbs), least significant first; the leaves are ordered most significant bit first.  bound: a public integer below
    2^L, None for p - 1 (the root is then [r >= p]).  One launch, no triple, no open, and no array of the bound."""
    bits, L, count = _sb_planes(ctx, bits)
    if bound is None:
        host = None
    else:
        if not (isinstance(bound, int) and not isinstance(bound, bool) and 0 <= bound < 1 << L):
            raise ValueError(f"bound: an integer in [0, 2^{L})")
        host = np.array([(bound >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(ctx.n_limbs)], dtype=np.uint64)
    g, p = ctx.torch.empty_like(bits), ctx.torch.empty_like(bits)
    rc = ctx.lib.hb_off_sb_leaves(ctx.h, ctx.ptr(bits), L, None if host is None else host.ctypes.data, ctx.ptr(g), ctx.ptr(p), count, ctx.stream())
    ctx.check(rc, "hb_off_sb_leaves")
    return g, p


def sb_finish(ctx, bits, index, check=True):
    """-> (r, r_bits), (len(index), limbs) and (L, len(index), limbs): slot j holds the planes of candidate index[j] and the residue
    r = sum_q 2^q b_q they compose, in one launch and one pass over the planes.  index: a contiguous int64 device tensor (k,), every
    entry in [0, count); anything else raises ValueError before any launch (the range check reads two words back: one
    synchronisation; check=False leaves it out for an index that torch.nonzero made)."""
    bits, L, count = _sb_planes(ctx, bits)
    t = ctx.torch
    if not isinstance(index, t.Tensor) or index.dtype != t.int64 or index.dim() != 1 or not index.is_cuda or index.device.index != ctx.device:
        raise ValueError(f"index: expected an int64 tensor of shape (k,) on cuda:{ctx.device}")
    if not index.is_contiguous():
        raise ValueError("index: must be contiguous")
    k = int(index.shape[0])
    if check and k and (int(index.min()) < 0 or int(index.max()) >= count):
        raise ValueError(f"index: every entry must lie in [0, {count})")
    r = ctx.empty(k)
    r_bits = t.empty((L, k, ctx.n_limbs), dtype=t.int64, device=ctx.tdev)
    rc = ctx.lib.hb_off_sb_finish(ctx.h, ctx.ptr(bits), L, count, ctx.ptr(index), ctx.ptr(r), ctx.ptr(r_bits), k, ctx.stream())
    ctx.check(rc, "hb_off_sb_finish")
    return r, r_bits


async def share_bits_round(co, bits, triples):
    """One round of rejection over given candidates: bits (L, m, limbs), this party's shares of m L random bits, least significant
    first, and triples = (p, q, pq), each (2 L - 3, m, limbs).  The leaves of [r > p - 1] (sb_leaves: affine, the bound is public),
    progs.fixedpoint.carry_tree over them -- carry_levels(L - 1) opens, carry_triples(L - 1) = 2 L - 3 rows of triples -- and ONE open
    of the root, the verdict w = [r >= p]: it tells of a discarded candidate that it was discarded, nothing else.  Every party sees
    the same verdicts, so torch.nonzero gives every party the same kept candidates in the same order, and sb_finish gathers their
    planes and composes r.  -> (r, r_bits, verdicts): (kept, limbs), (L, kept, limbs) and the public bool tensor [r_i < p], (m,).
    An opened verdict that is neither 0 nor 1 (a plane that was no bit) raises HoneyBadgerMPCError on every party.  m = 0 returns
    empty tensors without a launch.  The inputs are left untouched."""
    from .progs.fixedpoint import carry_tree

    ctx = co.ctx
    bits, L, m = _sb_planes(ctx, bits)
    t = ctx.torch
    if m == 0:
        return ctx.empty(0), t.empty((L, 0, ctx.n_limbs), dtype=t.int64, device=ctx.tdev), t.empty((0,), dtype=t.bool, device=ctx.tdev)
    g, p = sb_leaves(ctx, bits)
    root = await carry_tree(co, g, p, triples)
    w = await co.open_share_array(root)
    high_zero = (w[:, 1:] == 0).all(dim=1)
    verdicts = high_zero & (w[:, 0] == 0)
    rejected = high_zero & (w[:, 0] == 1)
    if not bool((verdicts | rejected).all()):
        raise HoneyBadgerMPCError("share bits: an opened verdict is neither 0 nor 1 (a bit plane did not hold a bit)")
    index = t.nonzero(verdicts).view(-1)
    r, r_bits = sb_finish(ctx, bits, index, check=False)
    return r, r_bits, verdicts


def _branch(co, name):
    """A coalescer of its own for one of several coroutines that run concurrently: OpenCoalescer numbers its batches in the order they
    are cut, and between concurrent coroutines that order depends on when messages arrive, which differs from party to party.  A
    branch has its own channels ((name, tag) on the parent's network) and its own numbering, in its own program order."""
    from .open_coalescer import OpenCoalescer

    parent = co.get_send_recv
    return OpenCoalescer(co.ctx.modulus, co.n, co.t, co.myid, lambda tag: parent((name, tag)), use_omega_powers=getattr(co, "use_omega_powers", False),
                         device=co.ctx.device)


async def _branches(co, tag, named):
    """named: [(name, f)] with f(branch) a coroutine -> the results, run concurrently, each on its own branch of co.  The first
    branch that raises ends the others: an abort of one randousha is an abort of the call, and nothing is left running."""
    kids = [_branch(co, (tag, name)) for name, _ in named]
    tasks = [asyncio.ensure_future(f(kid)) for kid, (_, f) in zip(kids, named)]
    try:
        return await asyncio.gather(*tasks)
    finally:
        for task in tasks:
            if not task.done():
                task.cancel()
        for kid in kids:                           # the parent's diagnostics count what ran on its behalf
            co.opens, co.batches = co.opens + kid.opens, co.batches + kid.batches


async def generate_share_bits(co, count, tag="share_bits", generator=None, chunk=1 << 14, bit_source=None, triple_source=None):
    """count random residues nobody knows, each shared together with its bit planes: (r, r_bits), (count, limbs) and (L, count, limbs),
    least significant first -- what share_comparison.less_than takes as r, r_bits (and s, s_bits), made among the parties.  Rejection
    sampling of a bitwise-shared value (share_bits_round): a round draws m = min(chunk, share_bits_candidates(p, still missing))
    candidates -- L m shared bits from bit_source(co, k, tag) (default generate_bits, ZERO_ONE) and (2 L - 3) m triples from
    triple_source(co, k, tag) (default generate_triples; its three (k, limbs) results are viewed as rows), the two running
    concurrently, each on a branch of co with its own channels and batch numbering -- keeps the candidates below p, and rounds repeat
    under the tags (tag, 0), (tag, 1), .. until there are enough; the surplus is dropped.  Over BLS12-381 (p / 2^255 = 0.9057) a kept
    residue costs about 282 bits and 560 triples; a round of any size is the two opens of generate_bits, the open of
    generate_triples, carry_levels(L - 1) tree levels and the verdicts' open.  Aborts are randousha's: anything but 2t successes
    raises HoneyBadgerMPCError in every party."""
    _positive_int(count, "generate_share_bits: count")
    _positive_int(chunk, "generate_share_bits: chunk")
    ctx = co.ctx
    p, L, nl = ctx.modulus, ctx.modulus.bit_length(), ctx.n_limbs
    if bit_source is None:
        def bit_source(co, k, tag):
            return generate_bits(co, k, encoding=ZERO_ONE, tag=tag, generator=generator)
    if triple_source is None:
        def triple_source(co, k, tag):
            return generate_triples(co, k, tag=tag, generator=generator)
    rows = 2 * L - 3
    kept_r, kept_bits, missing, rnd = [], [], count, 0
    while missing > 0:
        m = min(chunk, share_bits_candidates(p, missing))
        rtag = (tag, rnd)
        bits, trip = await _branches(co, rtag, [("bits", lambda kid: bit_source(kid, L * m, (rtag, "bits"))),
                                                ("triples", lambda kid: triple_source(kid, rows * m, (rtag, "triples")))])
        bits = ctx.elems(bits, L * m, what="bit_source's result").view(L, m, nl)
        try:
            tp, tq, tpq = trip
        except (TypeError, ValueError):
            raise ValueError("triple_source: expected (p, q, pq)") from None
        trip = tuple(ctx.elems(v, rows * m, what="triple_source's result").view(rows, m, nl) for v in (tp, tq, tpq))
        r, r_bits, _ = await share_bits_round(co, bits, trip)
        take = min(missing, int(r.shape[0]))
        kept_r.append(r[:take])
        kept_bits.append(r_bits[:, :take])
        missing -= take
        rnd += 1
    if len(kept_r) == 1 and kept_bits[0].is_contiguous():                     # one round that kept exactly count: nothing is copied
        return kept_r[0], kept_bits[0]
    return ctx.torch.cat(kept_r, dim=0).contiguous(), ctx.torch.cat(kept_bits, dim=1).contiguous()


LessThanPreprocessing = collections.namedtuple("LessThanPreprocessing", "r r_bits triples s s_bits")


async def generate_less_than_preprocessing(co, count, mode=HB_LT_DIRECT, tag="less_than_preprocessing", generator=None, chunk=1 << 14, bit_source=None,
                                           triple_source=None):
    """Everything share_comparison.less_than(co, a, b, r, r_bits, triples, s, s_bits, mode) consumes for `count` pairs, laid out as it
    takes it: r (count, limbs) and r_bits (L, count, limbs) from generate_share_bits; triples = (p, q, pq), each
    (less_than_triples(L, mode), count, limbs); s, s_bits a second pair in mode REFERENCE, None in DIRECT.  The generators run
    concurrently, each on a branch of co."""
    from .share_comparison import REFERENCE, _check_lt_mode, less_than_triples

    _check_lt_mode(mode)
    _positive_int(count, "generate_less_than_preprocessing: count")
    ctx = co.ctx
    L, nl = ctx.modulus.bit_length(), ctx.n_limbs
    rows = less_than_triples(L, mode)
    if triple_source is None:
        def triple_source(co, k, tag):
            return generate_triples(co, k, tag=tag, generator=generator)

    def share_bits(name):
        return lambda kid: generate_share_bits(kid, count, tag=(tag, name), generator=generator, chunk=chunk, bit_source=bit_source, triple_source=triple_source)

    named = [("r", share_bits("r")), ("triples", lambda kid: triple_source(kid, rows * count, (tag, "triples")))]
    if mode == REFERENCE:
        named.append(("s", share_bits("s")))
    got = await _branches(co, tag, named)
    (r, r_bits), trip = got[0], got[1]
    trip = tuple(ctx.elems(v, rows * count, what="triple_source's result").view(rows, count, nl) for v in trip)
    s, s_bits = got[2] if mode == REFERENCE else (None, None)
    return LessThanPreprocessing(r, r_bits, trip, s, s_bits)
