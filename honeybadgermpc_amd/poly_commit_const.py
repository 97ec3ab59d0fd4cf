"""
The PROVER of the reference's PolyCommitConst (poly_commit_const.py: the constant-size, KZG polynomial commitment HbAvssBatch uses) over
the fixed-base kernels of g1.py (csrc/hb_crs.hip).  commit and create_witness are sums of powers of the bases of the common reference
string, gs[j] = alpha^j g and hs[j] = alpha^j h, so they are pure G1; the reference-shaped methods keep its names and behaviour on host
objects (bls12_381.G1, the package's polynomials and field elements) and marshal into the batch calls, which are what a dealer uses.

The VERIFIER is not here.  verify_eval and batch_verify_eval compare pairings; this package has no G2 and no Fq12, so they raise
NotImplementedError and never return a verdict.  `ghats` (the G2 half of a reference CRS) is stored untouched and may be None.

There is no CPU path: without a GPU every method that computes raises HbmpcBackendError, like the rest of the package.

    crs = gen_pc_const_crs(t)                              [gs, None, hs], t + 1 bases a family
    pc = PolyCommitConst(crs)
    c, hat = pc.commit_batch(coeffs)                       coeffs (B, t + 1, 4) -> c (B, 2, 6), hat (B, t + 1, 4): ONE launch
    w, shares, aux = pc.witness_batch(coeffs, hat, xs)     n points -> w (B, n, 2, 6), shares (B, n, 4), aux (B, n, 4): THREE launches,
                                                           the whole double loop of HbAvssBatch._get_dealer_msg (hbavss.py:567-598)

What is NOT checked: that the bases are powers of one alpha (a CRS is trusted), that they lie in the subgroup of order R
(g1.in_subgroup tells), and that the coefficients handed in as tensors are canonical residues (ctx.reduce_ makes them so).
"""
import secrets

from . import g1
from ._capi import Context
from .bls12_381 import G1, R
from .field import GF
from .polynomial import polynomials_over

_NO_PAIRING = "needs a pairing (G2 and Fq12), which this package does not have: only the prover of PolyCommitConst runs here"


class PolyCommitConst(object):
    def __init__(self, pk, field=None, ctx=None, window=8):
        assert len(pk) == 3
        self.gs, self.ghats, self.hs = list(pk[0]), pk[1], list(pk[2])
        assert len(self.gs) == len(self.hs) and len(self.gs) >= 1
        for fam, w in ((self.gs, "gs"), (self.hs, "hs")):
            for p in fam:
                if not isinstance(p, G1):
                    raise TypeError(f"{w}: expected host G1 elements, got {type(p).__name__}")
        self.t = len(self.gs) - 1
        self.field = GF(R) if field is None else field
        if getattr(self.field, "modulus", None) != R:
            raise ValueError("field: the commitment's exponents live in GF(R), R = Subgroup.BLS12_381")
        self._ctx = ctx
        self.window = window
        self._tables = None

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

    def verify_eval(self, c, i, phi_at_i, phi_hat_at_i, witness):
        raise NotImplementedError(f"PolyCommitConst.verify_eval {_NO_PAIRING}")

    def batch_verify_eval(self, commits, i, shares, auxes, witnesses):
        raise NotImplementedError(f"PolyCommitConst.batch_verify_eval {_NO_PAIRING}")

    def preprocess_verifier(self, level=4):
        raise NotImplementedError(f"PolyCommitConst.preprocess_verifier {_NO_PAIRING}")


def gen_pc_const_crs(t, alpha=None, g=None, h=None, ctx=None):
    """-> [gs, None, hs]: gs[j] = alpha^j g, hs[j] = alpha^j h, j <= t, host G1; one batched g1.scalar_mul a family.  The middle entry is
    the reference's ghats, two points of G2, which this package cannot make.  alpha=None is drawn with `secrets` and not kept: whoever
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
    if ctx is None:
        ctx = Context.get(R)
    powers, run = [], 1
    for _ in range(t + 1):
        powers.append(run)
        run = run * alpha % R
    ks = ctx.upload_ints(powers)
    return [g1.download(g1.scalar_mul(ctx, ks, g)), None, g1.download(g1.scalar_mul(ctx, ks, h))]
