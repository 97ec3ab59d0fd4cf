"""
The reference's PolyCommitConst (poly_commit_const.py: the constant-size, KZG polynomial commitment HbAvssBatch uses), prover and verifier,
over the fixed-base kernels of g1.py (csrc/hb_crs.hip) and the pairing kernel of pairing.py (csrc/hb_pair.hip).  commit and
create_witness are sums of powers of the bases of the common reference string, gs[j] = alpha^j g and hs[j] = alpha^j h, so they are pure
G1; the reference-shaped methods keep its names and behaviour on host objects (bls12_381.G1, the package's polynomials and field
elements) and marshal into the batch calls, which are what a dealer and a recipient use.

The VERIFIER needs `ghats`, the G2 half of the CRS: [ghat, alpha ghat], host bls12_381_pairing.G2.  The reference's check
    e(c, ghat0) == e(w, ghat1 - i ghat0) e(g0, ghat0)^share e(h0, ghat0)^aux
is evaluated in the form
    e(c - share g0 - aux h0 + i w, ghat0) e(-w, ghat1) == 1
which needs no G2 operation and no power in GT: both G2 points are fixed by the CRS and PREPARED once on the host (pairing.PreparedG2),
the left side is G1 work for the kernels already here (msm_fixed over gs[0] and hs[0], scalar_mul, sub, add, neg: five launches,
each ending in an inversion an item: a tenth of a large batch's check), and one launch of k_pair_product runs two Miller loops that share their squarings and one final exponentiation.
A CRS without ghats (None in the middle) keeps the prover; the three verifier methods then raise NotImplementedError.

There is no CPU path: without a GPU every method that computes raises HbmpcBackendError, like the rest of the package.

    crs = gen_pc_const_crs(t, ghat=G2.generator())         [gs, ghats, hs], t + 1 bases a family; ghat=None: [gs, None, hs]
    pc = PolyCommitConst(crs)
    c, hat = pc.commit_batch(coeffs)                       coeffs (B, t + 1, 4) -> c (B, 2, 6), hat (B, t + 1, 4): ONE launch
    w, shares, aux = pc.witness_batch(coeffs, hat, xs)     n points -> w (B, n, 2, 6), shares (B, n, 4), aux (B, n, 4): THREE launches,
                                                           the whole double loop of HbAvssBatch._get_dealer_msg (hbavss.py:567-598)
    ok = pc.verify_batch(c, xs, shares, aux, w)            one verdict an item -> bool tensor (B,); xs one index or one an item
    ok = pc.verify_wire(c48, xs, shares, aux, w48)         the same from 48-byte compressed encodings, membership in the subgroup
                                                           checked: what a recipient runs on a dealer's message

What is NOT checked: that the bases are powers of one alpha and that ghats[1] = alpha ghats[0] for that same alpha (a CRS is trusted),
that the bases lie in the subgroup of order R, and that the scalars handed in as tensors are canonical residues (ctx.reduce_ makes
them so).  Membership of the commitments and the witnesses in that subgroup (the rearranged equation equals the reference's only
there) is checked when asked: verify_batch(..., check_subgroup=True) (off by default, as before) and verify_wire (on by default) run
the endomorphism test of csrc/hb_g1_wire.hip, one launch an array.
"""
import secrets

from . import g1, pairing
from ._capi import Context
from .bls12_381 import G1, R
from .bls12_381_pairing import G2
from .field import GF
from .polynomial import polynomials_over

_NO_PAIRING = "needs a pairing against ghats, and the G2 half of this CRS is missing (None): only the prover of PolyCommitConst runs on it"


class PolyCommitConst(object):
    def __init__(self, pk, field=None, ctx=None, window=8):
        assert len(pk) == 3
        self.gs, self.ghats, self.hs = list(pk[0]), pk[1], list(pk[2])
        assert len(self.gs) == len(self.hs) and len(self.gs) >= 1
        for fam, w in ((self.gs, "gs"), (self.hs, "hs")):
            for p in fam:
                if not isinstance(p, G1):
                    raise TypeError(f"{w}: expected host G1 elements, got {type(p).__name__}")
        if self.ghats is not None:
            self.ghats = list(self.ghats)
            if len(self.ghats) != 2 or not all(isinstance(p, G2) for p in self.ghats):
                raise TypeError("ghats: expected two host G2 elements, [ghat, alpha ghat], or None")
            if any(p.is_one() for p in self.ghats):
                raise ValueError("ghats: the identity pairs to 1 with everything")
        self.t = len(self.gs) - 1
        self.field = GF(R) if field is None else field
        if getattr(self.field, "modulus", None) != R:
            raise ValueError("field: the commitment's exponents live in GF(R), R = Subgroup.BLS12_381")
        self._ctx = ctx
        self.window = window
        self._tables = None
        self._vtables = None
        self._prepared = None

    # ---- plumbing
    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = Context.get(R)          # HbmpcBackendError without a GPU
        return self._ctx

    def preprocess_prover(self, level=8):
        """build the tables of gs and hs now (the reference's item.preprocess(level) over both families); level: the window width, 4 or 8"""
        self.window = level
        self._tables = None
        self.tables()

    def tables(self):
        if self._tables is None:
            ctx = self.ctx
            self._tables = (g1.FixedBases(ctx, self.gs, self.window), g1.FixedBases(ctx, self.hs, self.window))
        return self._tables

    def _coeffs(self, t, what):
        ctx = self.ctx
        t = ctx.elems(t, what=what)
        if t.dim() != 3 or t.shape[1] != self.t + 1:
            raise ValueError(f"{what}: expected a tensor of shape (B, t + 1, {ctx.n_limbs}) with t = {self.t}, got {tuple(t.shape)}")
        return t

    # ---- the batch calls
    def commit_batch(self, coeffs, hat=None):
        """coeffs (B, t + 1, 4): B polynomials' coefficients, canonical residues -> (c (B, 2, 6), hat (B, t + 1, 4)):
        c[b] = sum_j coeffs[b][j] * gs[j] + hat[b][j] * hs[j] in one launch.
        hat=None draws the blinding polynomials on the HOST with the `secrets` module and uploads them: torch's generators
        (torch.rand*, torch.Generator, on either device) are not cryptographic and must not blind a commitment."""
        ctx = self.ctx
        tg, th = self.tables()
        coeffs = self._coeffs(coeffs, "coeffs")
        B = int(coeffs.shape[0])
        if hat is None:
            hat = ctx.upload_ints([secrets.randbelow(R) for _ in range(B * (self.t + 1))]).reshape(B, self.t + 1, ctx.n_limbs)
        else:
            hat = self._coeffs(hat, "hat")
            if hat.shape[0] != B:
                raise ValueError(f"coeffs and hat: {B} polynomials against {int(hat.shape[0])}")
        return g1.msm_fixed(ctx, tg, coeffs, th, hat), hat

    def witness_batch(self, coeffs, hat, xs):
        """coeffs, hat (B, t + 1, 4) as commit_batch takes and returns them; xs: n points, a tensor (n, 4) or a list of ints ->
        (w (B, n, 2, 6), shares (B, n, 4), aux (B, n, 4)): w[b][i] the witness of the evaluation of polynomial b at xs[i],
        shares[b][i] = phi_b(xs[i]), aux[b][i] = hat_b(xs[i]).  Two quotient launches and one sum over gs[:t] and hs[:t].
        t = 0: the quotients are empty and every witness is the identity, as the reference's empty product is."""
        ctx = self.ctx
        tg, th = self.tables()
        coeffs, hat = self._coeffs(coeffs, "coeffs"), self._coeffs(hat, "hat")
        B = int(coeffs.shape[0])
        if hat.shape[0] != B:
            raise ValueError(f"coeffs and hat: {B} polynomials against {int(hat.shape[0])}")
        if not isinstance(xs, ctx.torch.Tensor):
            xs = ctx.upload_ints([int(x) % R for x in xs]).reshape(-1, ctx.n_limbs)
        q, shares = g1.kzg_quotients(ctx, coeffs, xs)
        qh, aux = g1.kzg_quotients(ctx, hat, xs)
        n = int(shares.shape[1])
        w = g1.msm_fixed(ctx, tg, q.reshape(B * n, self.t, ctx.n_limbs), th, qh.reshape(B * n, self.t, ctx.n_limbs))
        return w.reshape(B, n, 2, g1.LIMBS), shares, aux

    # ---- the reference's surface, on host objects
    def _host_coeffs(self, phi, what):
        cs = [int(c) % R for c in phi.coeffs]
        if len(cs) > self.t + 1:
            raise ValueError(f"{what}: degree {len(cs) - 1} is above the CRS's t = {self.t}")
        cs = cs + [0] * (self.t + 1 - len(cs))
        return self.ctx.upload_ints(cs).reshape(1, self.t + 1, self.ctx.n_limbs)

    def commit(self, phi):
        """-> (c, phi_hat): a host G1 and the blinding polynomial, as the reference returns them"""
        ctx = self.ctx
        c, hat = self.commit_batch(self._host_coeffs(phi, "phi"))
        phi_hat = polynomials_over(self.field)(ctx.download_ints(hat.reshape(self.t + 1, ctx.n_limbs)))
        return g1.download(c)[0], phi_hat

    def create_witness(self, phi, phi_hat, i):
        """-> the witness of phi(i), a host G1"""
        w, _, _ = self.witness_batch(self._host_coeffs(phi, "phi"), self._host_coeffs(phi_hat, "phi_hat"), [int(i)])
        return g1.download(w)[0]

    # ---- the verifier
    def _need_ghats(self, name):
        if self.ghats is None:
            raise NotImplementedError(f"PolyCommitConst.{name} {_NO_PAIRING}")

    def preprocess_verifier(self, level=4):
        """prepare ghats[0] and ghats[1] for the Miller loop and build the tables of gs[0] and hs[0] now (the reference's
        gg.preprocess(level), gh.preprocess(level)).  level: the window width of those two tables when it is 4 or 8, else ignored."""
        self._need_ghats("preprocess_verifier")
        if level in (4, 8) and level != self.window and self._tables is None:
            self.window = level
            self._vtables = None
        self._verifier_state()

    def _verifier_state(self):
        """-> (tables with gs[0], tables with hs[0], prepared ghats[0], prepared ghats[1])"""
        ctx = self.ctx
        if self._prepared is None:
            self._prepared = (pairing.PreparedG2(ctx, self.ghats[0]), pairing.PreparedG2(ctx, self.ghats[1]))
        if self._tables is not None:
            tg, th = self._tables
        else:
            if self._vtables is None:
                self._vtables = (g1.FixedBases(ctx, self.gs[:1], self.window), g1.FixedBases(ctx, self.hs[:1], self.window))
            tg, th = self._vtables
        return tg, th, self._prepared[0], self._prepared[1]

    def verify_lhs(self, commits, xs, shares, auxes, witnesses):
        """-> (A, -w), (B, 2, 6) each: A[b] = c[b] - shares[b] g0 - auxes[b] h0 + xs[b] w[b], composed from msm_fixed, scalar_mul
        and add.  Shapes as verify_batch."""
        self._need_ghats("verify_lhs")
        ctx = self.ctx
        tg, th, _, _ = self._verifier_state()
        c = g1._points(ctx, commits, what="commits")
        B = g1._n(c)
        w = g1._points(ctx, witnesses, B, what="witnesses")
        sh = ctx.elems(shares, B, what="shares").reshape(B, 1, ctx.n_limbs)
        au = ctx.elems(auxes, B, what="auxes").reshape(B, 1, ctx.n_limbs)
        if isinstance(xs, ctx.torch.Tensor):
            xs = ctx.elems(xs, what="xs")
            if xs.numel() // ctx.n_limbs not in (1, B):
                raise ValueError(f"xs: one index or {B}, got {xs.numel() // ctx.n_limbs}")
        elif isinstance(xs, (list, tuple)):
            if len(xs) not in (1, B):
                raise ValueError(f"xs: one index or {B}, got {len(xs)}")
            xs = ctx.upload_ints([int(x) % R for x in xs])
        else:
            xs = ctx.upload_ints([int(xs) % R])
        c, w = c.reshape(B, 2, g1.LIMBS), w.reshape(B, 2, g1.LIMBS)
        opened = g1.msm_fixed(ctx, tg, sh, th, au)
        lhs = g1.add(ctx, g1.sub(ctx, c, opened), g1.scalar_mul(ctx, xs, w)) if B else c
        return lhs, g1.neg(ctx, w)

    def verify_batch(self, commits, xs, shares, auxes, witnesses, check_subgroup=False):
        """commits (B, 2, 6), shares and auxes (B, 4), witnesses (B, 2, 6); xs: ONE index (an int, or a tensor (1, 4)) or one an item
        (a list of B ints, or a tensor (B, 4)) -> bool tensor (B,): verdict[b] = the reference's verify_eval(commits[b], xs[b],
        shares[b], auxes[b], witnesses[b]) for points of the subgroup of order R (see the module's head for what is not checked).
        Six launches: five for the left side in G1, one for two Miller loops and a final exponentiation an item.
        check_subgroup=True: two more launches, and an item whose commitment or witness is outside the subgroup is False."""
        self._need_ghats("verify_batch")
        ctx = self.ctx
        _, _, p0, p1 = self._verifier_state()
        lhs, nw = self.verify_lhs(commits, xs, shares, auxes, witnesses)
        ok, _ = pairing.product_is_one(ctx, [(lhs, p0), (nw, p1)])
        if check_subgroup:
            B = int(ok.shape[0])
            ok = ok & g1.in_subgroup(ctx, g1._points(ctx, commits, B, what="commits"), method="endomorphism") \
                & g1.in_subgroup(ctx, g1._points(ctx, witnesses, B, what="witnesses"), method="endomorphism")
        return ok

    def verify_wire(self, commits48, xs, shares, auxes, witnesses48, check_subgroup=True):
        """verify_batch for commitments and witnesses as they come from another party: 48-byte compressed encodings (what
        g1.decompress takes: uint8 (B, 48) on the device, or host bytes) -> bool tensor (B,).  Both arrays are decompressed with
        check_subgroup (one launch each, the membership test inside it), verify_batch runs on the results, and its verdicts are ANDed
        with status == 0 of both arrays: a malformed encoding or a point outside the subgroup is a False verdict, never an exception
        (a rejected item enters verify_batch as the identity)."""
        self._need_ghats("verify_wire")
        ctx = self.ctx
        c, cst, _ = g1.decompress(ctx, commits48, check_subgroup=check_subgroup)
        w, wst, _ = g1.decompress(ctx, witnesses48, check_subgroup=check_subgroup)
        if g1._n(c) != g1._n(w):
            raise ValueError(f"commits48 and witnesses48: {g1._n(c)} encodings against {g1._n(w)}")
        return self.verify_batch(c, xs, shares, auxes, w) & (cst == 0) & (wst == 0)

    def verify_eval(self, c, i, phi_at_i, phi_hat_at_i, witness):
        """-> bool, on host objects, as the reference's verify_eval"""
        self._need_ghats("verify_eval")
        ctx = self.ctx
        ok = self.verify_batch(g1.upload([c], ctx), int(i), ctx.upload_ints([int(phi_at_i) % R]), ctx.upload_ints([int(phi_hat_at_i) % R]),
                               g1.upload([witness], ctx))
        return bool(ok[0].item())

    def batch_verify_eval(self, commits, i, shares, auxes, witnesses):
        """-> bool, with the reference's semantics EXACTLY: ONE check of the product of the commitments and the product of the witnesses
        against the sums of the shares and of the auxes, all at index i.  There is NO random linear combination: errors that cancel
        in the sums pass, as they do in the reference; verify_batch gives a verdict an item.  An empty batch is True."""
        self._need_ghats("batch_verify_eval")
        commits, shares, auxes, witnesses = list(commits), list(shares), list(auxes), list(witnesses)
        assert len(commits) == len(shares) and len(commits) == len(witnesses) and len(commits) == len(auxes)
        n = len(commits)
        if n == 0:
            return True
        ctx = self.ctx
        ones = ctx.upload_ints([1] * n).reshape(1, n, ctx.n_limbs)
        cprod = g1.msm(ctx, ones, g1.upload(commits, ctx))
        wprod = g1.msm(ctx, ones, g1.upload(witnesses, ctx))
        ssum, asum = sum(int(v) for v in shares) % R, sum(int(v) for v in auxes) % R
        ok = self.verify_batch(cprod, int(i), ctx.upload_ints([ssum]), ctx.upload_ints([asum]), wprod)
        return bool(ok[0].item())


def gen_pc_const_crs(t, alpha=None, g=None, h=None, ctx=None, ghat=None):
    """-> [gs, ghats, hs]: gs[j] = alpha^j g, hs[j] = alpha^j h, j <= t, host G1; one batched g1.scalar_mul a family.  The middle entry is
    the reference's ghats: [ghat, ghat ** alpha] for a host G2 `ghat` (computed by the host model; not the identity), or None for
    ghat=None, which leaves a CRS for the prover alone.  alpha=None is drawn with `secrets` and not kept: whoever
    knows it can open a commitment to anything.  alpha = 0 mod R is refused: identity bases have no table.  g, h: default to two
    independent points derived from fixed seeds (the reference derives BOTH from one seed, so that h = g there)."""
    assert type(t) is int and t >= 0
    if alpha is None:
        alpha = 1 + secrets.randbelow(R - 1)
    alpha = int(alpha) % R
    if alpha == 0:
        raise ValueError("alpha: 0 mod R makes every base but the first the identity, which has no table")
    g = G1.rand([0, 0, 0, 1]) if g is None else g
    h = G1.rand([0, 0, 0, 2]) if h is None else h
    for p, w in ((g, "g"), (h, "h")):
        if not isinstance(p, G1):
            raise TypeError(f"{w}: expected a host G1, got {type(p).__name__}")
        if p.is_one():
            raise ValueError(f"{w}: the identity has no table")
    if ghat is not None:
        if not isinstance(ghat, G2):
            raise TypeError(f"ghat: expected a host G2, got {type(ghat).__name__}")
        if ghat.is_one():
            raise ValueError("ghat: the identity pairs to 1 with everything")
    if ctx is None:
        ctx = Context.get(R)
    powers, run = [], 1
    for _ in range(t + 1):
        powers.append(run)
        run = run * alpha % R
    ks = ctx.upload_ints(powers)
    ghats = None if ghat is None else [ghat, ghat ** alpha]
    return [g1.download(g1.scalar_mul(ctx, ks, g)), ghats, g1.download(g1.scalar_mul(ctx, ks, h))]
