"""Times the tiled scans (csrc/util.hip run_scan) of this build against other builds of the library, interleaved.

    python scripts/scan_ab.py [name=path/to/libcnrma_hip.so ...]

12 288 000 ints (the north-star shape's rays: the two scans of a scene) and 20 000 000 ints (beyond TILE^2 items: the
three-launch path), cnrma_exclusive_scan_i32 and cnrma_mask_to_index: one warm-up call, then six rounds of one call per
library in turn, HIP-event times in microseconds; the outputs of all libraries are compared."""
import ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cnrma_amd import _lib
from cnrma_amd._lib import ptr, stream

NAMES = ("cnrma_scan_workspace_bytes", "cnrma_exclusive_scan_i32", "cnrma_mask_to_index", "cnrma_abi_version")


def bind(path):
    lib = ctypes.CDLL(path)
    for name in NAMES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert lib.cnrma_abi_version() == _lib.ABI_VERSION
    return lib


dev = torch.device("cuda:0")
libs = {"this build": _lib.load()}
for arg in sys.argv[1:]:
    name, path = arg.split("=", 1)
    libs[name] = bind(path)
for n in (12_288_000, 20_000_000):
    count = torch.randint(0, 8, (n,), generator=torch.Generator(device=dev).manual_seed(1), dtype=torch.int32, device=dev)
    mask = (count > 3).to(torch.uint8)
    for what in ("exclusive_scan_i32", "mask_to_index"):
        series, outs = {}, {}
        for rep in range(7):
            for name, lib in libs.items():
                ws = torch.empty(lib.cnrma_scan_workspace_bytes(n), dtype=torch.uint8, device=dev)
                out = torch.empty(n + 1, dtype=torch.int32, device=dev)
                n_sel = torch.zeros(1, dtype=torch.int32, device=dev)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if what == "exclusive_scan_i32":
                    rc = lib.cnrma_exclusive_scan_i32(ptr(count), ptr(out), n, ptr(ws), stream())
                else:
                    rc = lib.cnrma_mask_to_index(ptr(mask), ptr(out), ptr(n_sel), n, ptr(ws), stream())
                b.record(); torch.cuda.synchronize()
                assert rc == 0
                if rep > 0:
                    series.setdefault(name, []).append(1e3 * a.elapsed_time(b))
                outs[name] = out[:n + (what == "exclusive_scan_i32")].clone()
        first = outs["this build"]
        for name, s in series.items():
            print(f"n {n} {what:20s} {name:12s} us:", [round(x, 1) for x in s], "median", round(statistics.median(s), 1),
                  "spread", round(max(s) - min(s), 1), "equal to this build:", torch.equal(outs[name], first))
