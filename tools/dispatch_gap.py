"""GPU diagnostic: the boundary between back-to-back scans, issued the way bench.py issues its steps (two slots on ONE
stream, step k+1 enqueued while step k runs, every count read back).
usage: rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/dispatch_gap.py run [launches] [pattern fixture]
       python3 tools/dispatch_gap.py parse DIR       start(k+1) - end(k) and kernel time of the full-size scan launches
       python3 tools/dispatch_gap.py both [launches] the boundary WITHOUT a tracer (under one, every dispatch carries a signal and
                                                     timestamps, whatever the library asks for): wall clock per launch minus
                                                     elapsed_ms, of the plain dispatch with the kernel's own clock and, in a
                                                     second process, of the dispatch with events (PFAC_EVENT_TIMING=1)"""
import glob, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(n_launch, name):
    os.environ.setdefault("PFAC_ENABLE_KNOBS", "1")
    sys.path.insert(0, ROOT)
    import torch
    from phfpfac_amd import GpuMatcher, PfacTable
    data = os.path.join(ROOT, "tests", "golden", "data")
    para = open(os.path.join(data, "paragraph402"), "rb").read()
    n = 1 << 30
    buf = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
    g = GpuMatcher(0, 2)
    g.set_stream(1, g.stream_handle(0))
    g.load_table(PfacTable.from_file(os.path.join(data, name), 256))
    g.fill_tiled(buf, n, para)
    g.reserve(0, 0, n // 8)
    g.reserve(1, 0, n // 8)
    first = g.scan_resident(n, n, d_input=buf)
    assert g.scan_resident(n, n, d_input=buf, slot=1) == first
    inflight = []
    for k in range(n_launch):
        g.scan_async(n, n, d_input=buf, slot=k & 1)
        inflight.append(k & 1)
        if len(inflight) == 2:
            assert g.scan_finish(inflight.pop(0))[0] == first
    while inflight:
        assert g.scan_finish(inflight.pop(0))[0] == first
    print(f"{n_launch} launches of {name} x 1 GiB, {first} matches each")


def parse(d):
    import csv
    import numpy as np
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)[-1]
    rows = [r for r in csv.DictReader(open(f)) if "pfac_scan_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    s = np.array([int(r["Start_Timestamp"]) for r in rows], dtype=np.int64)
    e = np.array([int(r["End_Timestamp"]) for r in rows], dtype=np.int64)
    dur = (e - s) / 1e3
    big = dur > 0.5 * np.median(dur)                     # the 1 GiB launches (not the heap-sizing ones at the start)
    s, e, dur = s[big], e[big], dur[big]
    s, e, dur = s[len(s) // 4:], e[len(e) // 4:], dur[len(dur) // 4:]      # steady state
    gap = (s[1:] - e[:-1]) / 1e3
    step = (s[-1] - s[0]) / 1e3 / (len(s) - 1)
    pct = lambda v: f"median {np.median(v):.2f} us, p10 {np.percentile(v, 10):.2f}, p90 {np.percentile(v, 90):.2f}"
    print(f"{os.path.basename(f)}: {len(s)} steady-state launches")
    print(f"  kernel: mean {dur.mean():.2f} us, {pct(dur)}")
    print(f"  start(k+1) - end(k): mean {gap.mean():.2f} us, {pct(gap)}")
    print(f"  start to start: {step:.2f} us per step")


if __name__ == "__main__":
    if sys.argv[1] == "both":
        for knob in ({}, {"PFAC_EVENT_TIMING": "1"}):
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "launch_wall.py"), sys.argv[2] if len(sys.argv) > 2 else "800", "2"],
                           env=dict(os.environ, PFAC_ENABLE_KNOBS="1", **knob), check=True)
    elif sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 200, sys.argv[3] if len(sys.argv) > 3 else "experimentpattern")
    else:
        parse(sys.argv[2])
