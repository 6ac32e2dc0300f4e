"""GPU diagnostic: bench.py's timed region many times over -- sync, 20 steps of the bench.py-shaped sequence (two slots on one
stream), drain, sync -- and how its ms_per_step is distributed: how often a 20-step window is slow, and whether in its kernels
or outside them.  usage: step_windows.py [windows]   (PFAC_HIP_LIB selects the build, PFAC_EVENT_TIMING=1 the dispatch with events)"""
import os, sys, time
os.environ.setdefault("PFAC_ENABLE_KNOBS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from phfpfac_amd import GpuMatcher, PfacTable
DATA = os.path.join(ROOT, "tests", "golden", "data")
para = open(os.path.join(DATA, "paragraph402"), "rb").read()
N = 1 << 30
tag = os.path.basename(os.environ.get("PFAC_HIP_LIB", "product")) + (" +events" if os.environ.get("PFAC_EVENT_TIMING") else "")
buf = torch.empty(N + 4096, dtype=torch.uint8, device="cuda:0")
with GpuMatcher(0, 2) as g:
    g.set_stream(1, g.stream_handle(0))
    g.load_table(PfacTable.from_file(os.path.join(DATA, "experimentpattern"), 256))
    g.fill_tiled(buf, N, para)
    g.reserve(0, 0, N // 8); g.reserve(1, 0, N // 8)
    first = g.scan_resident(N, N, d_input=buf)
    assert g.scan_resident(N, N, d_input=buf, slot=1) == first
    inflight, ms = [], []
    def fin():
        sl = inflight.pop(0); assert g.scan_finish(sl)[0] == first; ms.append(g.elapsed_ms(sl))
    def run(n):
        for k in range(n):
            g.scan_async(N, N, d_input=buf, slot=k & 1); inflight.append(k & 1)
            if len(inflight) == 2: fin()
        while inflight: fin()
    run(600)
    w, kk = [], []
    for i in range(int(sys.argv[1]) if len(sys.argv) > 1 else 300):
        ms.clear(); torch.cuda.synchronize(); t0 = time.perf_counter(); run(20); torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) / 20 * 1e6); kk.append(np.mean(ms) * 1e3)
    w, kk = np.array(w), np.array(kk)
    d = w - kk
    print(f"{tag}: window ms_per_step us p10 {np.percentile(w,10):.2f} p50 {np.median(w):.2f} p90 {np.percentile(w,90):.2f} p99 {np.percentile(w,99):.2f} max {w.max():.2f}; "
          f"kernel p10 {np.percentile(kk,10):.2f} p50 {np.median(kk):.2f} p90 {np.percentile(kk,90):.2f}; step-kernel p50 {np.median(d):.2f} p90 {np.percentile(d,90):.2f} p99 {np.percentile(d,99):.2f} max {d.max():.2f}; "
          f"windows with step-kernel > p50+3us: {(d > np.median(d) + 3).sum()} of {len(d)}", flush=True)
