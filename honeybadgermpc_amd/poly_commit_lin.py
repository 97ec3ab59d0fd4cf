"""
The reference's PolyCommitLin (poly_commit_lin.py: the linear, Pedersen polynomial commitment, the default scheme of HbAvssLight) over
the G1 kernels of g1.py.  The reference-shaped methods keep its names and behaviour on host objects (bls12_381.G1, the package's
polynomials and field elements) and marshal into the batch calls, which are what a protocol run uses: share arrays stay tensors.

There is no CPU path: without a GPU every method that computes raises HbmpcBackendError, like the rest of the package.

    crs = [G1.rand(seed_g), G1.rand(seed_h)]
    pc = PolyCommitLin(crs)
    cs, hat = pc.commit_batch(coeffs)                      coeffs (B, t + 1, 4) -> cs (B, t + 1, 2, 6), hat (B, t + 1, 4)
    ok = pc.verify_batch(cs, i, shares, witnesses)         (B,) bool tensor, recipient i
    pc.batch_verify_eval(cs, i, shares, witnesses)         one bool, read from the device's counter of rejected items

Witnesses.  The witness of recipient i for polynomial b is hat_b(i), so the witnesses of ALL recipients are the blinding polynomials
evaluated at 1..n -- the package's existing batched evaluation, not a kernel of this module:

    from honeybadgermpc_amd import ntl
    hat_rows = [ctx.download_ints(hat[b]) for b in range(B)]                # or keep the ints the dealer drew
    wit = ntl.vandermonde_batch_evaluate(list(range(1, n + 1)), hat_rows, R)  # wit[b][i - 1] = hat_b(i)

and the shares phi_b(i) come from the same call on the coefficients.

Sums over a list of commitments -- products of commitments, interpolation in the exponent (the reference's interpolate_g1_at_x) -- are
not methods of this class: g1.msm, g1.interpolate_at and g1.interpolate_g1_at_x work on the same (..., 2, 6) tensors.
"""
import secrets

from . import g1
from ._capi import Context
from .bls12_381 import G1, R
from .field import GF
from .polynomial import polynomials_over


class PolyCommitLin(object):
    def __init__(self, crs, field=None, ctx=None, window=8):
        assert len(crs) == 2
        self.g, self.h = crs
        for p, w in ((self.g, "crs[0]"), (self.h, "crs[1]")):
            if not isinstance(p, G1):
                raise TypeError(f"{w}: expected a host G1, got {type(p).__name__}")
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

    def preprocess(self, level=8):
        """build the fixed-base tables of g and h now (the reference's G1.preprocess(level)); level: the window width, 4 or 8"""
        self.window = level
        self._tables = None
        self.tables()

    def tables(self):
        if self._tables is None:
            ctx = self.ctx
            self._tables = (g1.FixedBase(ctx, self.g, self.window), g1.FixedBase(ctx, self.h, self.window))
        return self._tables

    # ---- the batch calls
    def commit_batch(self, coeffs, hat=None):
        """coeffs (B, t + 1, 4): B polynomials' coefficients, canonical residues -> (cs (B, t + 1, 2, 6), hat (B, t + 1, 4)):
        cs[b][j] = coeffs[b][j] * g + hat[b][j] * h in one launch.
        hat=None draws the blinding polynomials on the HOST with the `secrets` module and uploads them: torch's generators
        (torch.rand*, torch.Generator, on either device) are not cryptographic and must not blind a commitment."""
        ctx = self.ctx
        tg, th = self.tables()
        coeffs = ctx.elems(coeffs, what="coeffs")
        if coeffs.dim() != 3:
            raise ValueError(f"coeffs: expected a tensor of shape (B, t + 1, {ctx.n_limbs}), got {tuple(coeffs.shape)}")
        B, n_coef = int(coeffs.shape[0]), int(coeffs.shape[1])
        if hat is None:
            hat = ctx.upload_ints([secrets.randbelow(R) for _ in range(B * n_coef)]).reshape(B, n_coef, ctx.n_limbs)
        else:
            hat = ctx.elems(hat, B * n_coef, what="hat").reshape(B, n_coef, ctx.n_limbs)
        cs = g1.commit(ctx, tg, th, coeffs.reshape(B * n_coef, ctx.n_limbs), hat.reshape(B * n_coef, ctx.n_limbs))
        return cs.reshape(B, n_coef, 2, g1.LIMBS), hat

    def verify_batch(self, cs, i, shares, witnesses):
        """-> (B,) bool tensor: item b holds iff sum_j i^j cs[b][j] == shares[b] * g + witnesses[b] * h (and its commitments are on
        the curve).  One launch; nothing synchronises."""
        tg, th = self.tables()
        verdict, _ = g1.verify(self.ctx, tg, th, cs, i, shares, witnesses)
        return verdict != 0

    # ---- the reference's surface, on host objects
    def commit(self, phi):
        degree = len(phi.coeffs) - 1
        ctx = self.ctx
        coeffs = ctx.upload_ints([int(c) for c in phi.coeffs]).reshape(1, degree + 1, ctx.n_limbs)
        cs, hat = self.commit_batch(coeffs)
        phi_hat = polynomials_over(self.field)(ctx.download_ints(hat.reshape(degree + 1, ctx.n_limbs)))
        return g1.download(cs), phi_hat

    def create_witness(self, aux, i):
        return aux(i)

    def verify_eval(self, cs, i, phi_at_i, witness):
        return self.batch_verify_eval([cs], i, [phi_at_i], [witness])

    def batch_verify_eval(self, commits, i, shares, witnesses):
        """lists of host objects as the reference takes them, or the tensors of verify_batch -> one bool (the device counts the
        rejected items; reading the counter is the one synchronisation)"""
        ctx = self.ctx
        t = ctx.torch
        if not isinstance(commits, t.Tensor):
            assert len(commits) == len(shares) and len(commits) == len(witnesses)
            if len(commits) == 0:
                return True
            n_coef = max(len(c) for c in commits)
            flat = [p for c in commits for p in list(c) + [G1.one()] * (n_coef - len(c))]
            commits = g1.upload(flat, ctx).reshape(len(commits), n_coef, 2, g1.LIMBS)
        if not isinstance(shares, t.Tensor):
            shares = ctx.upload_ints([int(s) % R for s in shares])
        if not isinstance(witnesses, t.Tensor):
            witnesses = ctx.upload_ints([int(w) % R for w in witnesses])
        tg, th = self.tables()
        _, counter = g1.verify(ctx, tg, th, commits, int(i), shares, witnesses)
        return int(counter.item()) == 0
