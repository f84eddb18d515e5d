"""bench.py's options and the size of what --dump-outputs writes, without a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_bench_has_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in p.stdout, opt


def test_dump_positions_are_fixed_and_bounded():
    import bench
    budget, size = (1920 * 1080 // 2 + 7) // 8, 3 * 1080 * 1920
    for batch in (1, 4, 256, 1000):
        spos, dpos = bench.dump_positions(batch, budget, size)
        again = bench.dump_positions(batch, budget, size)
        assert (spos == again[0]).all() and (dpos == again[1]).all()
        assert len(set(spos.tolist())) == spos.size and 0 <= spos.min() and spos.max() < budget
        assert len(set(dpos.tolist())) == dpos.size and 0 <= dpos.min() and dpos.max() < size
        # the two sampled arrays (float32 bytes, float64 values) and the small per-image ones stay under 64 MB
        assert batch * (4 * spos.size + 8 * dpos.size + 8 * 5) <= 64 << 20
