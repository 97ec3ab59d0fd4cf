"""Every mat-vec reduction, and the element-wise, NTT and robust-decoder kernels, driven at edge-valued inputs AND edge-valued outputs
(tests/edge_values.py): coefficients that are pool values, polynomials interpolated in Python ints so that the encode's outputs, the
inputs of the decode's 1/den scaling and the values a validation compares are pool values (0, p - 1, 2^bits - p, all-ones words and
digits, the int8 sign boundary).  Exact equality against Python ints; the C oracle only where Python would be too slow (transforms above
order 64, the robust decoders).

Shapes (n, t): (64, 21) -- 22 rows: a full and a short row tile --, (24, 5), (16, 5) at omega powers, (7, 2); len(pool) + 3 chunks: every
value at every position, and a ragged count that is no multiple of 16.  Omega-power points exist where 32 divides p - 1 (BLS, secp256k1's
group order, Goldilocks).  Parametrised by (modulus, path) so that a failure names the kernel."""
import functools
import os
import random

import pytest

import edge_values as ev
import oracle
from conftest import BLS, clear_hook, set_hook

pytestmark = pytest.mark.gpu

SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P256, P64, GOLDILOCKS = (1 << 256) - 189, (1 << 64) - 59, 0xFFFFFFFF00000001
WIDE = [BLS, P256, SECP_N, (1 << 255) - 19, (1 << 255) + 95]
WIDE_IDS = ["bls", "2^256-189", "secp256k1-n", "2^255-19", "2^255+95"]
NARROW = [P64, GOLDILOCKS, (1 << 61) - 1]
NARROW_IDS = ["2^64-59", "goldilocks", "2^61-1"]
SHAPES = [(64, 21, False), (24, 5, False), (16, 5, True), (7, 2, False)]


def _ctx(p):
    from honeybadgermpc_amd._capi import Context

    return Context.get(p)


def _flat(rows):
    return [v for r in rows for v in r]


def _party_major(vals, n):
    """[chunk][point] -> the flat [point][chunk] layout of an encode's output and a decode's input"""
    return [vals[k][j] for j in range(n) for k in range(len(vals))]


def _split(n, t):
    """the decoded, the compared and the remaining columns of a shape"""
    order = list(range(n))
    random.Random(n * 100 + t).shuffle(order)
    return order[: t + 1], order[t + 1 : 2 * t + 1], order[2 * t + 1 :]


@functools.lru_cache(maxsize=None)
def _reference(p, x, t):
    """everything the paths of one (modulus, shape) share, computed once in Python ints and left unchanged"""
    n, d = len(x), t + 1
    x = list(x)
    count = len(ev.edge_pool(p, ev.n_limbs_of(p))) + 3
    z, zc, rest = _split(n, t)
    ref = {"z": z, "zc": zc, "rest": rest, "count": count}
    ref["edge"] = ev.edge_rows(p, d, count, seed=n)
    ref["edge_vals"] = ev.evaluate_rows(p, x, ref["edge"])
    ref["at_z"] = ev.targeted_rows(p, x, z, d, count, seed=1)
    ref["at_z_vals"] = ev.evaluate_rows(p, x, ref["at_z"])
    ref["at_zc"] = ev.targeted_rows(p, x, zc + [z[0]], d, count, seed=2)
    ref["at_zc_vals"] = ev.evaluate_rows(p, x, ref["at_zc"])
    return ref


@functools.lru_cache(maxsize=None)
def _full_size_image(p, x, t):
    """whether the full-size kernel can hold this plan's matrices [V^-1(z) ; V[zc] V^-1(z)]: an entry of its int8 image is 32 balanced
    base-256 digits (hb_mfma_wide.hip, mm8w_from_host), which every residue fits when the top byte of p is at most 0x7e (the rule of the
    images built on the device, hb_quick.hip) and otherwise only the entries below about 0x7f80.. do -- in Python ints: the columns of
    V^-1(z) are the Lagrange basis at the decoded points, V[zc] V^-1(z) their values at the compared ones.  Where it cannot, a plan asked
    for the full-size kernel says so (fused_validate_kernel() is None) and serves the call on its other kernels: the cases still run.
    This repeats a rule of the implementation inside the test, the price of asserting which kernel served instead of accepting either
    answer: if the image's digits change (entries taken as v - p, say), this prediction has to follow, whatever the kernels compute."""
    if p >> 248 <= 0x7E:
        return True
    z, zc, _ = _split(len(x), t)
    xs = [x[j] for j in z]
    basis = [ev.interpolate(p, xs, [int(i == j) for i in range(t + 1)]) for j in range(t + 1)]
    compared = ev.evaluate_rows(p, [x[j] for j in zc], basis)
    return all(ev.fits_32_balanced_digits(v) for row in basis + compared for v in row)


def _alterations(p, v, bits, rnd):
    """+1, -1 and one flipped bit in each 32-bit word, every result below p and different from v (a word of zeros of p - 1, as over
    Goldilocks and 2^255 + 95, in which every flip passes p, is left out)"""
    out = [(v + 1) % p, (v - 1) % p]
    for w in range(bits // 32):
        for b in rnd.sample(range(32), 32):
            nv = v ^ (1 << (32 * w + b))
            if nv < p:
                out.append(nv)
                break
    assert len(out) >= 3 and all(nv != v and 0 <= nv < p for nv in out)
    return out


def _four_cases(op, p, t, label):
    """cases 1 to 4 of one plan whose switches are set: `label` names the modulus, shape and path in a failure"""
    ctx = op.ctx
    n, d = op.n, t + 1
    bits = 64 * ctx.n_limbs
    ref = _reference(p, tuple(op.x), t)
    z, zc, rest, c = ref["z"], ref["zc"], ref["rest"], ref["count"]
    b = c * d
    # case 1: edge inputs, encode -- every output
    got = ctx.download_ints(op.r1_encode(ctx.upload_ints(_flat(ref["edge"]))))
    assert got == _party_major(ref["edge_vals"], n), (label, "encode of edge rows")
    # case 2: edge outputs, encode -- the outputs at z are the pool values themselves
    got = ctx.download_ints(op.r1_encode(ctx.upload_ints(_flat(ref["at_z"]))))
    tg = ev.targets(p, d, c, seed=1)
    assert all(got[j * c + k] == tg[k][i] for k in range(c) for i, j in enumerate(z)), (label, "encode onto pool values")
    assert got == _party_major(ref["at_z_vals"], n), (label, "encode of targeted rows")
    # case 3: edge outputs, decode
    cols = ctx.upload_ints(_party_major(ref["edge_vals"], n))
    res, msg = op.r2_decode(cols, b), op.r1_decode(cols, b)
    assert op.ok(), (label, "decode to edge rows")
    assert ctx.download_ints(res) == _flat(ref["edge"]) and ctx.download_ints(msg) == [r[0] for r in ref["edge"]], (label, "decode to edge rows")
    # case 4: edge inputs of the 1/den scaling (pool values in the decoded columns), then edge values at every compared point
    for rows, vals, what in ((ref["at_z"], ref["at_z_vals"], "pool values decoded"), (ref["at_zc"], ref["at_zc_vals"], "pool values compared")):
        cols = ctx.upload_ints(_party_major(vals, n))
        res, msg = op.r2_decode(cols, b), op.r1_decode(cols, b)
        assert op.ok(), (label, what)
        assert ctx.download_ints(res) == _flat(rows) and ctx.download_ints(msg) == [r[0] for r in rows], (label, what)
    # ... and an altered compared value is refused, the same alteration of a column nobody compares is not (cols: pool values compared)
    tg = ev.targets(p, d, c, seed=2)
    rnd = random.Random(n + t)
    for s_i, special in enumerate((0, p - 1, ((1 << bits) - p) % p)):
        i = s_i % t
        k = next(k for k in range(c) if tg[k][i] == special)
        assert ref["at_zc_vals"][k][zc[i]] == special
        for col, caught in ((zc[i], True), (rest[0], False)):
            v = ref["at_zc_vals"][k][col]
            for a_i, nv in enumerate(_alterations(p, v, bits, rnd)):
                bad = cols.clone()
                bad[col * c + k] = ctx.upload_ints([nv])[0]
                (op.r1_decode if a_i == 0 else op.r2_decode)(bad, b)
                assert op.ok() != caught, (label, special, col, hex(nv))


def _shapes(p, omega_too=True, min_d=1):
    return [(n, t, om) for n, t, om in SHAPES if t + 1 >= min_d and (not om or (omega_too and (p - 1) % 32 == 0))]


# ---- the wide (four-limb) mat-vec kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["k_mm8", "k_mm8f", "k_mm8w", "valu"])
@pytest.mark.parametrize("p", WIDE, ids=WIDE_IDS)
def test_wide_open_at_edge_values(p, path):
    """k_mm8: small-integer points, encode, decode and validating re-encode on the small-entry kernel (fusion off).  k_mm8f: the same plans
    decoding + validating in one launch of the small-entry kernel with the division inside.  k_mm8w: the id asks for the full-size
    kernel -- "wide" at small-integer points, the default at omega powers, fused and unfused -- and gets it where its image can hold the
    plan's matrices (_full_size_image: every plan over BLS, the (24, 5) plan over the two moduli around 2^255).  Over 2^256 - 189 and
    secp256k1's order no plan gets it: those two ids assert that the plan says so and then run the cases on what serves instead (k_mm8
    in two launches; the integer kernels at omega powers): at the moduli next to 2^256, the only ones where the full-size reduction's
    remainder can reach 2^256, tests/test_gpu_wide_matvec.py drives it through hb_matvec over matrices of its own.  Under this id only
    the decodes run k_mm8w: small points encode on k_mm8, omega plans by NTT, and the full-size encode needs large points that are no
    omega powers, which no shape here has.  The balanced launch k_mm8w_flat takes 49 rows or more of 57 coefficients or more and some
    thousand chunks (mm8w_flat_slots): that test has it too.
    valu: the integer-VALU kernels (matrix cores off), every shape."""
    from honeybadgermpc_amd.device import BatchOpen

    if path != "valu" and os.environ.get("HB_NO_MFMA"):
        pytest.skip("matrix-core path disabled by HB_NO_MFMA")
    pool_len = len(ev.edge_pool(p, 4))
    for n, t, om in _shapes(p, omega_too=path in ("k_mm8w", "valu"), min_d=4 if path in ("k_mm8f", "k_mm8w") else 1):
        if om and path == "k_mm8w":
            settings = [True, False]                    # omega powers: full-size entries whatever is asked; fused and unfused
        else:
            settings = {"k_mm8": [False], "k_mm8f": [True], "k_mm8w": ["wide"], "valu": [False]}[path]
        for fused in settings:
            z, zc, _ = _split(n, t)
            op = BatchOpen(p, n, t, z=z, zc=zc, use_omega_powers=om, max_shares=(pool_len + 3) * (t + 1))
            op.set_matrix_cores(path != "valu")
            op.set_fused_validate(fused)
            wide = _full_size_image(p, tuple(op.x), t)
            # (a plan at omega powers has no other matrix-core kernel: without the image it is on the integer kernels altogether)
            assert op.uses_matrix_cores() == (path != "valu" and (wide or not om)), (n, t, om)
            want = {"k_mm8": None, "k_mm8f": "small", "k_mm8w": "wide" if fused and wide else None, "valu": None}[path]
            assert op.fused_validate_kernel() == want, (n, t, om, fused)
            _four_cases(op, p, t, (path, n, t, om, fused))


# ---- the narrow (one-limb) mat-vec kernels ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["k_mv64m", "k_mv64", "valu"])
@pytest.mark.parametrize("p", NARROW, ids=NARROW_IDS)
def test_narrow_open_at_edge_values(p, path, monkeypatch):
    """k_mv64m (the 8-byte mat-vec on the matrix cores) and k_mv64 (the same plan with HB_NO_MFMA=1, the hook
    test_narrow_matrix_core_kernel_equals_the_integer_kernel uses); valu: the plan told to leave them (the generic integer kernels).  A
    narrow plan reports the 8-byte mat-vec as its one-launch decode + validate and nothing finer: WHICH of the two kernels ran is not
    asserted, it rests on the hook and on k_mv64m's conditions (hb_narrow.hip, mv64_matrix_cores: at most 24 coefficients, p >= 2^41),
    which the shapes and moduli here are checked to meet."""
    from honeybadgermpc_amd.device import BatchOpen

    if path == "k_mv64":
        set_hook(monkeypatch, "HB_NO_MFMA", "1")
    else:
        if os.environ.get("HB_NO_MFMA") and path == "k_mv64m":
            pytest.skip("matrix-core path disabled by HB_NO_MFMA")
        clear_hook(monkeypatch, "HB_NO_MFMA")
    pool_len = len(ev.edge_pool(p, 1))
    for n, t, om in _shapes(p, omega_too=path != "k_mv64"):      # (omega powers without the matrix cores are not the 8-byte mat-vec's)
        z, zc, _ = _split(n, t)
        op = BatchOpen(p, n, t, z=z, zc=zc, use_omega_powers=om, max_shares=(pool_len + 3) * (t + 1))
        op.set_matrix_cores(path != "valu")
        assert op.ctx.n_limbs == 1 and t + 1 <= 24 and p >> 41
        assert op.uses_fused_validate() == (path != "valu"), (n, t, om)
        _four_cases(op, p, t, (path, n, t, om))


# ---- case 5: element-wise and program kernels -----------------------------------------------------------------------------
def _operands(p):
    return ev.operands(p, ev.n_limbs_of(p))


@pytest.mark.parametrize("p", [BLS, P256, P64], ids=["bls", "2^256-189", "2^64-59"])
def test_share_arithmetic_every_ordered_pair(p):
    import itertools

    from honeybadgermpc_amd import share_arithmetic as sa

    ctx = _ctx(p)
    vs = _operands(p)
    pairs = list(itertools.product(vs, repeat=2))
    a, b = ctx.upload_ints([x for x, _ in pairs]), ctx.upload_ints([y for _, y in pairs])
    assert ctx.download_ints(sa.add(ctx, a, b)) == [(x + y) % p for x, y in pairs]
    assert ctx.download_ints(sa.sub(ctx, a, b)) == [(x - y) % p for x, y in pairs]
    assert ctx.download_ints(sa.mul(ctx, a, b)) == [x * y % p for x, y in pairs]
    one = ctx.upload_ints(vs)
    assert ctx.download_ints(sa.neg(ctx, one)) == [-x % p for x in vs]
    for s in (0, 1, p - 1, ((1 << (64 * ctx.n_limbs)) - p) % p, vs[len(vs) // 2]):      # the broadcast forms
        assert ctx.download_ints(sa.add(ctx, one, s)) == [(x + s) % p for x in vs]
        assert ctx.download_ints(sa.sub(ctx, one, s)) == [(x - s) % p for x in vs]
        assert ctx.download_ints(sa.mul(ctx, one, s)) == [x * s % p for x in vs]
    nz = [v for v in vs if v]
    assert ctx.download_ints(sa.inv(ctx, ctx.upload_ints(nz))) == [pow(x, -1, p) for x in nz]
    inverses, zeros = sa.inv(ctx, one, check=False)
    assert ctx.download_ints(inverses) == [pow(x, -1, p) if x else 0 for x in vs] and int(zeros.item()) == 1
    ts = list(itertools.product(ev.reduced_pool(p, ctx.n_limbs), repeat=5))
    cols = [ctx.upload_ints([tp[k] for tp in ts]) for k in range(5)]
    assert ctx.download_ints(sa.beaver_combine(ctx, *cols)) == [(d * e + d * q + e * pp + pq) % p for d, e, pp, q, pq in ts]


@pytest.mark.parametrize("p", [BLS, P64], ids=["bls", "2^64-59"])
def test_mimc_kernels_at_pool_values(p):
    from honeybadgermpc_amd.progs import mimc
    from test_gpu_mimc import _round_ref

    ctx = _ctx(p)
    vs = _operands(p)
    m = len(vs)
    xs, ks = vs, [vs[(7 * i + 3) % m] for i in range(m)]
    want = [mimc.mimc_plain(x, k, p) for x, k in zip(xs, ks)]
    x_dev, k_dev = ctx.upload_ints(xs), ctx.upload_ints(ks)
    for pair in (False, True):
        assert ctx.download_ints(mimc.mimc_plain_device(ctx, x_dev, k_dev, pair=pair)) == want, pair
    rot = lambda s: [vs[(i * s + s) % m] for i in range(m)]  # noqa: E731
    y, r, r2, r3, key, rn = vs, rot(3), rot(5), rot(7), rot(11), rot(13)
    dev = [ctx.upload_ints(v) for v in (y, r, r2, r3, key, rn)]
    for ctr in (0, 160):
        got = mimc.cube_round(ctx, dev[0], dev[1], dev[2], dev[3], dev[4], ctr, r_next=dev[5])
        assert ctx.download_ints(got) == [_round_ref(p, *tp[:4], tp[4], ctr, tp[5]) for tp in zip(y, r, r2, r3, key, rn)], ctr
        got = mimc.cube_round(ctx, dev[0], dev[1], dev[2], dev[3], p - 1, ctr)
        assert ctx.download_ints(got) == [_round_ref(p, *tp, p - 1, ctr, None) for tp in zip(y, r, r2, r3)], ctr


# ---- case 6: the transforms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [8, 64, 512, 4096])
@pytest.mark.parametrize("p", [BLS, GOLDILOCKS], ids=["bls", "goldilocks"])
def test_ntt_at_edge_values(p, order):
    """one, two, three and four radix-8 passes of the LDS kernel, and -- bls-4096 alone -- the four-step transform (4096 elements of 36 bytes
    with their twiddles do not fit the LDS; Goldilocks' 12-byte elements do, so goldilocks-4096 is still the LDS kernel: the four-step on
    1-limb contexts is test_gpu_ntt.py's): coefficients that are pool values, and coefficients chosen by the inverse transform so that the
    OUTPUTS are pool values"""
    from honeybadgermpc_amd import ntl

    g = next(a for a in range(2, 1000) if pow(a, (p - 1) // 2, p) != 1)
    omega = pow(g, (p - 1) // order, p)
    assert pow(omega, order // 2, p) == p - 1
    pool = ev.edge_pool(p, ev.n_limbs_of(p))
    count = len(pool) + 3 if order <= 64 else (8 if order == 512 else 3)
    rows = ev.edge_rows(p, order, count, seed=order)

    def forward(rs, w):
        if order <= 64:
            return ev.evaluate_rows(p, [pow(w, i, p) for i in range(order)], rs)
        return [oracle.fft(r, w, p, order) for r in rs]

    assert ntl.fft_batch_evaluate(rows, omega, p, order, order) == forward(rows, omega)
    ninv = pow(order, -1, p)
    back = [[v * ninv % p for v in r] for r in forward(rows, pow(omega, -1, p))]
    assert ntl.fft_batch_evaluate(back, omega, p, order, order) == rows


# ---- case 7: the robust decoders ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, n, k", [(BLS, 64, 22), (P256, 31, 11), (P64, 40, 10)], ids=["bls-64-22", "2^256-189-31-11", "2^64-59-40-10"])
def test_robust_decoders_at_edge_values(p, n, k):
    from honeybadgermpc_amd import ntl
    from honeybadgermpc_amd.device import wb_decode_batch

    rnd = random.Random(n * k)
    pool = ev.edge_pool(p, ev.n_limbs_of(p))
    x = list(range(1, n + 1))
    emax = (n - k) // 2
    rows = ev.edge_rows(p, k, 24, seed=k)
    clean = ev.evaluate_rows(p, x, rows)
    for pool_errors in (False, True):
        words = []
        for w in clean:
            w = list(w)
            for j in rnd.sample(range(n), emax):
                new = rnd.choice(pool) if pool_errors and rnd.random() < 0.5 else rnd.randrange(p)
                w[j] = new if new != w[j] else (new + 1) % p
            words.append(w)
        got = ntl.gao_interpolate_batch(x, words, k, p)
        assert got == oracle.gao_interpolate_batch(x, words, k, p), pool_errors
        assert all(co is not None for co, _ in got)
        got = wb_decode_batch(x, k, words, p)
        assert got == oracle.wb_decode_batch(x, k, words, p), pool_errors
        assert all(st == 0 for _, st in got)
