"""The merge-exchange network of progs/sorting.py checked on the CPU, from scratch (no import of the package):
   python scratch/merge_exchange_model.py

Enumerates the (p, r, d) layers of Knuth 5.2.2 Algorithm M, builds each layer's pairs from the closed form lo(e) and the closed cnt,
asserts they equal the filtered enumeration and form a matching, runs all 0/1 inputs for n <= 13 and random inputs up to 257, and
compares the layer and comparator counts at n = 2^j."""
import itertools
import random


def network(n):
    if n < 2:
        return []
    t = (n - 1).bit_length()
    out = []
    for a in range(t - 1, -1, -1):
        p = 1 << a
        out.append((p, 0, p))
        out.extend((p, p, (1 << j) - p) for j in range(t - 1, a, -1))
    return out


def closed(n, p, r, d):
    a = p.bit_length() - 1
    full, rem = divmod(max(n - d, 0), 2 * p)
    cnt = full * p + (min(rem, p) if r == 0 else max(rem - p, 0))
    return [(((e >> a) << (a + 1)) | (e & (p - 1)) | r, (((e >> a) << (a + 1)) | (e & (p - 1)) | r) + d) for e in range(cnt)]


def run(n, v):
    for p, r, d in network(n):
        for lo, hi in closed(n, p, r, d):
            if v[lo] >= v[hi]:
                v[lo], v[hi] = v[hi], v[lo]
    return v


for n in range(0, 300):
    for p, r, d in network(n):
        pairs = closed(n, p, r, d)
        assert pairs == [(i, i + d) for i in range(max(n - d, 0)) if i & p == r], (n, p, r, d)
        rows = [i for pair in pairs for i in pair]
        assert len(set(rows)) == len(rows) and all(0 <= lo < hi < n for lo, hi in pairs)
for n in range(0, 14):
    for bits in itertools.product((0, 1), repeat=n):
        assert run(n, list(bits)) == sorted(bits), (n, bits)
rnd = random.Random(1)
for n in (14, 31, 64, 100, 255, 256, 257):
    v = [rnd.randrange(50) for _ in range(n)]
    assert run(n, list(v)) == sorted(v), n
for j in range(1, 11):
    layers = [closed(1 << j, *l) for l in network(1 << j)]
    assert len(layers) == j * (j + 1) // 2 and sum(map(len, layers)) == (j * j - j + 4) * (1 << j) // 4 - 1
for n in (5, 13, 1000, 1024):
    layers = [c for c in (closed(n, *l) for l in network(n)) if c]
    print(n, len(layers), sum(map(len, layers)))
