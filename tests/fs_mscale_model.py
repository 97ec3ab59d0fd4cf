"""Big-integer model of k_mm8f's division of a received element by den_l on the matrix cores (hb_mfma_fused.hip, scale_unit's MSCALE
branch): the tables the builder writes per term, the int8 contraction, the gathering of its 32 columns and the one-word Barrett tail,
with every bound the kernel relies on as an assertion.  CPU only; tests/test_fs_mscale_model.py runs it.

For term l, w = 1 / den_l mod p and y = sum_b y_b 256^b the 32 bytes of a received element:

    y w = sum_b y_b U[b]  (mod p),   U[b] = 256^b w mod p  as 32 balanced base-256 digits (of U[b] or of U[b] - p)

    column c = CINIT[c] + sum_b (y_b - 128) digit_c(U[b]),   CINIT[c] = 2^20 + byte c of K,   K = (128 sum_b U[b] - sum_c 2^20 256^c) mod p

so that sum_c column_c 256^c = y w (mod p) with every column positive.  CINIT is the C operand of the first MFMA of a column quad."""

BIAS = 1 << 20


def balanced_digits(t, n=32):
    """n balanced base-256 digits of t (may be negative); None if it does not fit"""
    out = []
    for _ in range(n):
        d = t & 0xff
        if d > 127:
            d -= 256
        out.append(d)
        t = (t - d) >> 8
    return out if t == 0 else None


def term_tables(p, w):
    """(digits[b][c], cinit[c]) of the term with 1 / den = w"""
    assert 0 < w < p and 1 << 254 <= p < 1 << 256
    digits = []
    for b in range(32):
        u = (w << (8 * b)) % p
        dg = balanced_digits(u)
        if dg is None:
            dg = balanced_digits(u - p)
        assert dg is not None, "no 32-digit representative"
        assert sum(x << (8 * c) for c, x in enumerate(dg)) % p == u
        digits.append(dg)
    # (the kernel's builder: K = w * (128 * sum_b 256^b) - btot mod p, one Montgomery product and one subtraction)
    btot = sum(BIAS << (8 * c) for c in range(32))
    k = (w * (128 * sum(1 << (8 * b) for b in range(32))) - btot) % p
    cinit = [BIAS + ((k >> (8 * c)) & 0xff) for c in range(32)]
    return digits, cinit


def scale_model(y, p, tab, facts=None):
    """the representative of y w mod p that the kernel writes to LDS: below 2p where p < 2^255, canonical otherwise"""
    digits, cinit = tab
    assert 0 <= y < 1 << 256
    h = [((y >> (8 * b)) & 0xff) - 128 for b in range(32)]            # the bytes XOR 0x80, read as int8
    assert all(-128 <= x <= 127 for x in h)
    cols = []
    for c in range(32):
        # two MFMAs chained on one accumulator: bytes 0-15, then 16-31; int32 at every step, the constant included
        acc = cinit[c]
        for half in range(2):
            acc += sum(h[b] * digits[b][c] for b in range(16 * half, 16 * half + 16))
            assert -(1 << 31) <= acc < 1 << 31
        assert BIAS - (1 << 19) <= acc < 2 * BIAS + 256 and acc > 0
        cols.append(acc)
    # words: lo = c0 + c1 2^8 and hi = c2 + c3 2^8 are 32-bit sums without overflow, the word is lo + 2^16 hi in 64 bits
    P = []
    for k in range(8):
        lo = cols[4 * k] + (cols[4 * k + 1] << 8)
        hi = cols[4 * k + 2] + (cols[4 * k + 3] << 8)
        assert lo < 1 << 32 and hi < 1 << 32
        v = lo + (hi << 16)
        assert v < 1 << 46
        P.append(v)
    R = sum(v << (32 * k) for k, v in enumerate(P))
    assert R < 1 << 271
    w = sum(x << (8 * c) for c, x in enumerate(digits[0])) % p                # (U[0] = w)
    assert R % p == y * w % p
    # the one-word quotient of FS_REDUCE: mu = floor(2^286 / p)
    mu = (1 << 286) // p
    assert mu < 1 << 32
    tq = P[7] + (P[6] >> 32)
    rtop = tq >> 16
    assert rtop < 1 << 32
    q = (rtop * mu) >> 46
    assert q in (R // p, R // p - 1), (q, R // p)
    assert q < 1 << 18
    pneg = (1 << 256) - p
    u = [P[k] + q * ((pneg >> (32 * k)) & 0xffffffff) for k in range(8)]
    assert all(x < 1 << 64 for x in u)
    rp = sum(x << (32 * k) for k, x in enumerate(u))
    r = rp - (q << 256)
    assert 0 <= r < 2 * p
    top = (rp >> 256) - q
    assert top in (0, 1) and top == r >> 256
    if facts is not None:
        facts.add("exact" if q == R // p else "under")
        facts.add("top%d" % top)
    if p >> 255:
        # r < 2p may pass 2^256: the conditional subtraction of scale_unit (carry out of r + pneg, or bit 256)
        low = r & ((1 << 256) - 1)
        take = (low + pneg) >> 256 or top
        assert bool(take) == (r >= p)
        if take:
            r -= p
        assert r < p
    assert r < 1 << 256 and r % p == y * w % p
    return r


def inv_den(p, xs, j):
    """1 / prod_{q != j} (xs[j] - xs[q]) mod p"""
    den = 1
    for q, x in enumerate(xs):
        if q != j:
            den = den * (xs[j] - x) % p
    return pow(den, -1, p)
