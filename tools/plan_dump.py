"""GPU diagnostic: what an upload decides, one line per (table, knob set) -- the PFAC_VERBOSE line of the install, info(),
and the record width of a 64 KiB scan.  Two builds that print the same lines plan every one of these tables alike.
usage: plan_dump.py   (PFAC_HIP_LIB selects the build, as in tools/ab_kernel.sh)"""
import gzip, os, sys, tempfile
os.environ.setdefault("PFAC_ENABLE_KNOBS", "1")     # tuning / test knobs of libpfac_hip.so are opt-in
os.environ["PFAC_VERBOSE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phfpfac_amd import GpuMatcher, PfacTable
from phfpfac_amd.matcher import tiled_bytes
DATA = os.path.join(ROOT, "tests", "golden", "data")
TABLES = ["experimentpattern", "bytefile_10000byte", "xaa", "xaa+xab+xac+xad", "bytefile_1000000byte.gz"]
KNOBS = [{}, {"PFAC_FORCE_L2": "1"}, {"PFAC_FORCE_L2": "1", "PFAC_NO_FUSE": "1"}, {"PFAC_NO_D1": "1"}, {"PFAC_NO_D1PACK": "1"},
         {"PFAC_WIDE": "1"}, {"PFAC_DENSE": "1"}, {"PFAC_LAG": "1"}, {"PFAC_NWB": "4"}, {"PFAC_L2F": "0"}, {"PFAC_L2F": "2"},
         {"PFAC_L2F": "3"}]
ALL_KNOBS = sorted({k for ks in KNOBS for k in ks})


def pattern_bytes(name):
    if name.endswith(".gz"):
        return gzip.open(os.path.join(DATA, name), "rb").read()
    return b"".join(open(os.path.join(DATA, p), "rb").read() for p in name.split("+"))


def stderr_of(call):
    """What `call` writes to file descriptor 2 (the library prints there, not through sys.stderr)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode()


data = tiled_bytes(1 << 16, open(os.path.join(DATA, "paragraph402"), "rb").read())
with tempfile.TemporaryDirectory() as tmp:
    for name in TABLES:
        path = os.path.join(tmp, "patterns")
        open(path, "wb").write(pattern_bytes(name))
        table = PfacTable.from_file(path, 256)
        for knobs in KNOBS:
            for k in ALL_KNOBS:                     # (an install reads the knobs anew)
                os.environ.pop(k, None)
            os.environ.update(knobs)
            with GpuMatcher(0, 1) as g:
                lines = [l for l in stderr_of(lambda: g.load_table(table)).splitlines() if l.startswith("pfac: variant")]
                info = g.info()
                n = g.scan_bytes(data).size
                rec_bytes = g.scan_format()[0]
            tag = "+".join(f"{k}={v}" for k, v in knobs.items()) or "-"
            print(f"{name} [{tag}]: {' | '.join(lines)} || {info} || record bytes {rec_bytes}, {n} matches", flush=True)
