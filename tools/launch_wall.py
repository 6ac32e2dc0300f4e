"""GPU diagnostic: wall-clock time per scan of the bench.py-shaped sequence (two slots on ONE stream, step k+1 enqueued while
step k runs, every count and every elapsed_ms read back) -- what the boundary between two scans costs shows here and in no
kernel time.  usage: launch_wall.py [launches per pass] [passes] [pattern fixture]
PFAC_HIP_LIB selects the build (tools/ab_kernel.sh), PFAC_EVENT_TIMING=1 the dispatch with events.  One line per pass."""
import os, sys, time
os.environ.setdefault("PFAC_ENABLE_KNOBS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from phfpfac_amd import GpuMatcher, PfacTable

n_launch = int(sys.argv[1]) if len(sys.argv) > 1 else 800
n_pass = int(sys.argv[2]) if len(sys.argv) > 2 else 2
name = sys.argv[3] if len(sys.argv) > 3 else "experimentpattern"
DATA = os.path.join(ROOT, "tests", "golden", "data")
para = open(os.path.join(DATA, "paragraph402"), "rb").read()
N = 1 << 30
tag = os.path.basename(os.environ.get("PFAC_HIP_LIB", "product")) + (" +events" if os.environ.get("PFAC_EVENT_TIMING") else "")
buf = torch.empty(N + 4096, dtype=torch.uint8, device="cuda:0")
with GpuMatcher(0, 2) as g:
    g.set_stream(1, g.stream_handle(0))
    g.load_table(PfacTable.from_file(os.path.join(DATA, name), 256))
    g.fill_tiled(buf, N, para)
    g.reserve(0, 0, N // 8)
    g.reserve(1, 0, N // 8)
    first = g.scan_resident(N, N, d_input=buf)
    assert g.scan_resident(N, N, d_input=buf, slot=1) == first
    inflight, ms = [], []

    def finish_oldest():
        sl = inflight.pop(0)
        assert g.scan_finish(sl)[0] == first
        ms.append(g.elapsed_ms(sl))

    def run(n):
        for k in range(n):
            g.scan_async(N, N, d_input=buf, slot=k & 1)
            inflight.append(k & 1)
            if len(inflight) == 2:
                finish_oldest()
        while inflight:
            finish_oldest()

    run(400)                                           # clocks settle
    for p in range(n_pass):
        ms.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(n_launch)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / n_launch * 1e6
        kern = float(np.mean(ms)) * 1e3
        print(f"{tag} {name} pass {p}: wall {wall:.2f} us per launch, elapsed_ms mean {kern:.2f} us, "
              f"wall - elapsed {wall - kern:.2f} us ({n_launch} launches)", flush=True)
