"""
From power sums to messages on the device (csrc/hb_rf.hip): the reference's apps/asynchromix/solver/solver.py:20 solve() and the
FLINT program behind it (apps/asynchromix/solver/solver.cpp), on the (count, limbs) int64 tensors the rest of the package speaks.
With power_mixing.power_mix in front, this is the reference's async_mixing (apps/asynchromix/powermixing.py) end to end.

    solve(ctx, sums, seed=0)                    -> list[int], the k messages ascending, with multiplicity; or None
    roots(ctx, coeffs, seed=0)                  -> (k, limbs) tensor of the roots of a monic polynomial, ascending; or None
    newton_coefficients_device(ctx, sums)       -> (k + 1, limbs), bit-equal to power_mixing.newton_coefficients
    async mix(co, a_shares, powers, method="auto", seed=0)   -> power_mix, then solve

None is the reference's RET_INVALID: the sums are not the power sums of k field elements (the polynomial has a factor of degree
above one).  That is decided, never assumed: for a squarefree s and h = (x + a)^((p-1)/2) mod s, the degrees of gcd(s, h - 1),
gcd(s, h + 1) and gcd(s, h) add up to deg s exactly when s is a product of distinct linear factors, and the library counts them at
every node's first draw.  ValueError is its RET_INPUT_ERROR: k < 2, a modulus not above k, k above MAX_K.

MAX_K = 1024 (the reference's cap is 4097).  A polynomial GCD runs in one workgroup with both remainders in the LDS of one
compute unit: 2 (k + 1) coefficients of 36 bytes, 74 KB of the unit's 160 KB at k = 1024 -- two such workgroups a unit -- and the
k x k table that reduces a product modulo the top node is 38 MB.  It is also the largest size the tests run.

Repeated roots: roots(f) = distinct(f / g) ++ roots(g) with g = gcd(f, f') (f' != 0 because p > k), so the library takes as many
rounds -- a GCD, a division and a wait each -- as the largest multiplicity.  Distinct roots are split level by level; nodes of
degree at most SMALL_DEGREE take one launch a level, larger ones two launches for each bit of (p - 1) / 2.  hb_rf_roots owns that
loop and waits for the stream once a level: `roots` and `solve` return finished results.

`seed` chooses the random shifts (a counter-based generator on (seed, level, node, draw)); the result does not depend on it.
Without a GPU every function here raises HbmpcBackendError, like the rest of the package.
"""
import ctypes

from ._capi import HB_ERR_HIP, HB_RF_MAX_K, HB_RF_SMALL_DEGREE
from .power_mixing import power_mix

MAX_K = HB_RF_MAX_K
SMALL_DEGREE = HB_RF_SMALL_DEGREE


def _check_k(k, modulus):
    if k < 2:
        raise ValueError(f"at least two power sums (k >= 2), got {k}")
    if modulus <= k:
        raise ValueError(f"k = {k} needs a modulus above k")
    if k > MAX_K:
        raise ValueError(f"k = {k} is above solver.MAX_K = {MAX_K}")


def _sums_tensor(ctx, sums):
    """list of ints or (k, limbs) tensor -> k (checked) and the tensor (None while `sums` is still a list)"""
    if isinstance(sums, (list, tuple)):
        _check_k(len(sums), ctx.modulus)
        return len(sums), None
    shape = getattr(sums, "shape", None)
    if shape is None or len(shape) != 2 or int(shape[1]) != ctx.n_limbs:
        raise ValueError(f"sums: expected a list of ints or a tensor of shape (k, {ctx.n_limbs})")
    _check_k(int(shape[0]), ctx.modulus)
    return int(shape[0]), sums


def newton_coefficients_device(ctx, sums):
    """The monic polynomial with power sums S_1 .. S_k, coefficient of x^i at row i: Newton's identities in one launch of one
    workgroup (k dependent steps).  Bit-equal to power_mixing.newton_coefficients, the host model.  Asynchronous on the current stream."""
    if isinstance(sums, (list, tuple)):
        if len(sums) < 1 or ctx.modulus <= len(sums) or len(sums) > MAX_K:
            raise ValueError("sums: 1 <= k <= MAX_K and k below the modulus")
        sums = ctx.upload_ints([int(v) for v in sums])
    k = int(sums.shape[0]) if getattr(sums, "dim", lambda: 0)() == 2 else -1
    if k < 1 or ctx.modulus <= k or k > MAX_K:
        raise ValueError(f"sums: expected a tensor of shape (k, {ctx.n_limbs}), 1 <= k <= MAX_K and k below the modulus")
    sums = ctx.elems(sums, k, what="sums")
    out = ctx.empty(k + 1)
    ctx.check(ctx.lib.hb_rf_newton(ctx.h, ctx.ptr(sums), k, ctx.ptr(out), ctx.stream()), "hb_rf_newton")
    return out


def roots(ctx, coeffs, seed=0):
    """The k roots of the monic polynomial `coeffs` ((k + 1, limbs), coefficient of x^i at row i) as a (k, limbs) tensor, ascending,
    with multiplicity; None when it is not a product of k linear factors.  Waits for the stream (once a level of the split tree)."""
    t = ctx.torch
    if not isinstance(coeffs, t.Tensor) or coeffs.dim() != 2 or int(coeffs.shape[0]) < 2:
        raise ValueError(f"coeffs: expected a tensor of shape (k + 1, {ctx.n_limbs})")
    k = int(coeffs.shape[0]) - 1
    if ctx.modulus <= k:
        raise ValueError(f"degree {k} needs a modulus above it")
    if k > MAX_K:
        raise ValueError(f"degree {k} is above solver.MAX_K = {MAX_K}")
    coeffs = ctx.elems(coeffs, k + 1, what="coeffs")
    if ctx.download_ints(coeffs[k:]) != [1]:
        raise ValueError("coeffs: the polynomial must be monic")
    out = ctx.empty(k)
    n = ctypes.c_int32(0)
    rc = ctx.lib.hb_rf_roots(ctx.h, ctx.ptr(coeffs), k, ctypes.c_uint64(int(seed) & (2**64 - 1)), ctx.ptr(out), ctypes.byref(n), ctx.stream())
    if rc == HB_ERR_HIP:
        msg = ctx.lib.hb_last_error(ctx.h)
        if msg and msg.decode().startswith("hb_rf_roots:"):
            raise RuntimeError(msg.decode())
    ctx.check(rc, "hb_rf_roots")
    if n.value < 0:
        return None
    # k <= MAX_K canonical elements: sorted on the host
    return ctx.upload_ints(sorted(ctx.download_ints(out)))


def solve(ctx, sums, seed=0):
    """The k messages whose power sums are S_1 .. S_k (a list of ints or a (k, limbs) tensor), as Python ints in ascending order with
    multiplicity; None when the sums are not the power sums of k field elements.  Newton's identities, `roots`, unpacking."""
    k, tensor = _sums_tensor(ctx, sums)           # (needs ctx.modulus and ctx.n_limbs alone: ValueError comes before any device call)
    if tensor is None:
        tensor = ctx.upload_ints([int(v) for v in sums])
    found = roots(ctx, newton_coefficients_device(ctx, tensor), seed=seed)
    return None if found is None else ctx.download_ints(found)


async def mix(co, a_shares, powers, method="auto", seed=0):
    """The reference's async_mixing on tensors over an OpenCoalescer: the opened power sums of the shared messages
    (power_mixing.power_mix), then solve -- every party obtains the sorted messages, and nobody learns who sent which."""
    sums = await power_mix(co, a_shares, powers, method=method)
    return solve(co.ctx, sums, seed=seed)
