"""
Power mixing on the device (csrc/hb_pm.hip): phases 1-3 of the reference's apps/asynchromix/powermixing.py:12-95 and the NTL
program it shells out to once a client (apps/asynchromix/cpp/compute-power-sums.cpp), on the (count, limbs) int64 tensors the
rest of the package speaks.  No files, no subprocess.

For each of M clients the parties hold shares of a message a and of the powers b, b^2, ..., b^k of a random b (preprocessing).
c = a - b is opened; then

    [a^m] = sum_{j <= m} C(m, j) c^(m-j) [b^j]            ([b^0] = 1)

is a local, linear map of the shares: with u_j = [b^j] / j! and v_i = c^i / i!, [a^m] / m! = (u * v)[m], a convolution.  The
power sums S_m = sum over clients of a^m are opened and Newton's identities turn them into the polynomial whose roots are the
messages -- the shuffle: nobody learns which client sent which.

    powers_from_masked(ctx, a_minus_b, powers)                 -> (M, k)  this party's shares of a_c^1 .. a_c^k
    local_power_sums(ctx, a_minus_b, powers, method="auto")    -> (k,)    this party's shares of S_1 .. S_k
    async power_mix(co, a_shares, powers, method="auto")       -> (k,)    the opened power sums
    newton_coefficients(sums, modulus)                         -> list[int], coefficient of x^i at [i], monic, degree len(sums)

`a_minus_b`: (M, limbs), public; `powers`: (M, k, limbs), this party's shares, row c = b_c^1 .. b_c^k.  method: "direct" (a tiled
triangular convolution, any prime above k), "ntt" (transforms of order N = the power of two above 2k; needs N | p - 1), "auto"
(the library's crossover between the two).  Everything runs on torch's current stream and nothing synchronises, except that the
first call for a given k builds the factorial tables.  Finding the roots of the polynomial (the reference's FLINT solver,
apps/asynchromix/solver/solver.cpp) is honeybadgermpc_amd.solver: solver.solve takes the opened sums to the messages, solver.mix
runs power_mix and solve; newton_coefficients below is the host model of its first step.
"""
from ._capi import HB_ERR_UNSUPPORTED, HB_PM_AUTO, HB_PM_DIRECT, HB_PM_NTT, np_ptr
from .field import GF
from .share_arithmetic import sub

_METHODS = {"auto": HB_PM_AUTO, "direct": HB_PM_DIRECT, "ntt": HB_PM_NTT}
_OMEGAS = {}        # (modulus, order) -> omega as host limbs: get_omega is a full-size exponentiation on Python ints, 0.6 ms over BLS12-381


def _omega(ctx, order):
    key = (ctx.modulus, ctx.n_limbs, order)
    if key not in _OMEGAS:
        from .polynomial import get_omega

        _OMEGAS[key] = ctx.host_elems([int(get_omega(GF(ctx.modulus), order, seed=0).value)])
    return _OMEGAS[key]


def transform_order(k):
    """the power of two above 2k: the length the convolution of two (k + 1)-vectors needs"""
    n = 1
    while n <= 2 * k:
        n *= 2
    return n


def _operands(ctx, a_minus_b, powers):
    t = ctx.torch
    if not isinstance(powers, t.Tensor) or powers.dim() != 3:
        raise ValueError(f"powers: expected a tensor of shape (clients, k, {ctx.n_limbs})")
    m, k = int(powers.shape[0]), int(powers.shape[1])
    if k < 1:
        raise ValueError("powers: at least one power a client (k >= 1)")
    if k >= ctx.modulus:
        raise ValueError(f"k = {k} powers need a modulus above k (j! must be invertible for j <= k)")
    powers = ctx.elems(powers, m * k, what="powers")
    a_minus_b = ctx.elems(a_minus_b, m, what="a_minus_b")
    return a_minus_b, powers, m, k


def powers_from_masked(ctx, a_minus_b, powers):
    """This party's shares of a_c^m, m = 1 .. k, for every client c (what computePowers returns, compute-power-sums.cpp:17-84)."""
    a_minus_b, powers, m, k = _operands(ctx, a_minus_b, powers)
    out = ctx.torch.empty((m, k, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    ctx.check(ctx.lib.hb_pm_powers(ctx.h, ctx.ptr(a_minus_b), ctx.ptr(powers), m, k, ctx.ptr(out), ctx.stream()), "hb_pm_powers")
    return out


def local_power_sums(ctx, a_minus_b, powers, method="auto"):
    """This party's shares of S_m = sum_c a_c^m, m = 1 .. k (the .sums file of the reference's phase 2)."""
    if method not in _METHODS:
        raise ValueError(f"method: one of {sorted(_METHODS)}, got {method!r}")
    a_minus_b, powers, m, k = _operands(ctx, a_minus_b, powers)
    order = transform_order(k)
    omega_ptr, n = None, 0
    if method != "direct" and (ctx.modulus - 1) % order == 0 and order <= 1 << 22:
        omega_ptr, n = np_ptr(_omega(ctx, order)), order
    elif method == "ntt":
        raise ValueError(f"method='ntt': the field has no root of unity of order {order} (the power of two above 2k)")
    out = ctx.torch.empty((k, ctx.n_limbs), dtype=ctx.torch.int64, device=ctx.tdev)
    rc = ctx.lib.hb_pm_power_sums(ctx.h, ctx.ptr(a_minus_b), ctx.ptr(powers), m, k, _METHODS[method], omega_ptr, n, ctx.ptr(out), ctx.stream())
    if rc == HB_ERR_UNSUPPORTED and method == "ntt":
        raise ValueError("method='ntt': not available for this k")
    ctx.check(rc, "hb_pm_power_sums")
    return out


async def power_mix(co, a_shares, powers, method="auto"):
    """The opened power sums S_1 .. S_k of the M shared messages `a_shares` ((M, limbs)), using one row of `powers` a message:
    open(a - b), the local power sums, open(sums) -- powermixing.py:12-95 without its files and its k subprocesses.  Every party
    runs the same coroutine over its OpenCoalescer."""
    ctx = co.ctx
    if not isinstance(powers, ctx.torch.Tensor) or powers.dim() != 3:
        raise ValueError(f"powers: expected a tensor of shape (clients, k, {ctx.n_limbs})")
    a_minus_b = await co.open_share_array(sub(ctx, a_shares, powers[:, 0].contiguous()))
    sums = local_power_sums(ctx, a_minus_b, powers, method=method)
    return await co.open_share_array(sums)


def newton_coefficients(sums, modulus):
    """The monic polynomial prod_c (x - a_c) from the power sums S_1 .. S_k of its k roots, by Newton's identities
    m e_m = sum_{i=1..m} (-1)^(i-1) e_(m-i) S_i; returned as Python ints, the coefficient of x^i at index i (so [k] == 1).
    k^2 / 2 products through field.py on the host: sequential by nature, and small beside the opens.  Needs modulus > k."""
    field = GF(modulus)
    k = len(sums)
    if k < 1:
        raise ValueError("at least one power sum")
    if k >= modulus:
        raise ValueError("Newton's identities divide by 1 .. k: the modulus must be above k")
    s = [None] + [field(int(v)) for v in sums]
    e = [field(1)]
    for m in range(1, k + 1):
        acc = field(0)
        for i in range(1, m + 1):
            term = e[m - i] * s[i]
            acc = acc + term if i % 2 else acc - term
        e.append(acc * ~field(m))
    # prod (x - a_c) = sum_m (-1)^m e_m x^(k-m)
    return [int((e[k - i] if (k - i) % 2 == 0 else -e[k - i]).value) for i in range(k + 1)]
