"""bench.py --dump-outputs without a GPU: dump_outputs() writes field elements as float64 rows of their 32-bit words, other integer
arrays as they are, and a large output as the same seeded sample every time, with its element indices beside it.  Run in a child
process: importing bench sets OpenMP variables for the process that imports it."""
import subprocess
import sys

from conftest import REPO

_CODE = r"""
import os, sys
import numpy as np
import bench

out_dir = sys.argv[1]
rng = np.random.Generator(np.random.PCG64(5))
small = rng.integers(-(1 << 63), (1 << 63) - 1, size=(1000, 4), dtype=np.int64)
big = rng.integers(-(1 << 63), (1 << 63) - 1, size=(bench.DUMP_ROWS + 12345, 4), dtype=np.int64)
status = np.arange(bench.DUMP_ROWS + 7, dtype=np.int32) % 3
for sub in ("a", "b"):
    bench.dump_outputs(os.path.join(out_dir, sub), {"small": small, "big": big, "status": status})

def ints(words):
    return [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in words]

def load(sub, name):
    return np.load(os.path.join(out_dir, sub, name + ".npy"))

s = load("a", "small")
assert s.dtype == np.float64 and s.shape == (1000, 8)
assert ints(s) == ints(small.view(np.uint32))
assert not os.path.exists(os.path.join(out_dir, "a", "small_index.npy"))
b, bi = load("a", "big"), load("a", "big_index")
assert b.dtype == np.float64 and b.shape == (bench.DUMP_ROWS, 8) and bi.shape == (bench.DUMP_ROWS,)
idx = bi.astype(np.int64)
assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < big.shape[0]
assert ints(b[:50]) == ints(big[idx[:50]].view(np.uint32))
st, sti = load("a", "status"), load("a", "status_index")
assert st.shape == (bench.DUMP_ROWS, 1) and (st[:, 0] == status[sti.astype(np.int64)]).all()
for name in os.listdir(os.path.join(out_dir, "a")):
    assert np.array_equal(load("a", name[:-4]), load("b", name[:-4])), name
total = sum(os.path.getsize(os.path.join(out_dir, "a", f)) for f in os.listdir(os.path.join(out_dir, "a")))
assert total <= bench.DUMP_BYTES
print("dump ok")
"""


def test_dump_outputs_format_and_sample(tmp_path):
    res = subprocess.run([sys.executable, "-c", _CODE, str(tmp_path)], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "dump ok" in res.stdout
