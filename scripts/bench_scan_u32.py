"""Time sw_scan_u32 alone (HIP events around one call) at the sizes of the re-key partition's
[world][ptiles] count matrix, ptiles taken at the benchmark's rec_cap and carry_cap.  Prints one
JSON line.  SW_GPU_LIB selects the library under test; --zero-tmp clears the scratch before every
call (outside the timed region), for a build whose scan needs that.

    python scripts/bench_scan_u32.py --worlds 8,64 --calls 48
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="8,64", help="n = world x ptiles for each")
    ap.add_argument("--msgs", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--zero-tmp", action="store_true")
    a = ap.parse_args()
    import torch
    from sitewhere_amd._native import gpu, gpu_library_path
    from sitewhere_amd.pipeline.config import EngineConfig
    lib = gpu()
    d = torch.device("cuda", 0)
    s = torch.cuda.current_stream(d)
    P = ctypes.c_void_p
    cfg = EngineConfig(max_msgs=a.msgs, rec_cap=a.msgs + 4096, world=8)      # bench.py's sizing, 8 ranks
    ptiles = (cfg.carry_cap + cfg.rec_cap + 1023) // 1024
    out = {"bench": "scan_u32", "lib": os.environ.get("SW_GPU_LIB") or str(gpu_library_path()), "zero_tmp": a.zero_tmp, "ptiles": ptiles, "sizes": []}
    for w in (int(x) for x in a.worlds.split(",")):
        n = w * ptiles
        x = np.random.default_rng(w).integers(0, 8192, n, dtype=np.int64).astype(np.uint32)
        xin = torch.from_numpy(x.view(np.int32)).to(d)
        res = torch.zeros(n, dtype=torch.int32, device=d)
        tmp = torch.zeros(2 * (n // 1024 + 4), dtype=torch.int32, device=d)
        us = []
        for k in range(a.warmup + a.calls):
            if a.zero_tmp:
                tmp.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            rc = lib.sw_scan_u32(P(xin.data_ptr()), n, P(res.data_ptr()), None, P(tmp.data_ptr()), tmp.numel(),
                                 P(s.cuda_stream))
            e1.record(s)
            e1.synchronize()
            assert rc == 0, rc
            if k >= a.warmup:
                us.append(1000.0 * e0.elapsed_time(e1))
        want = np.concatenate([np.zeros(1, np.uint32), np.cumsum(x, dtype=np.uint32)[:-1]])
        assert np.array_equal(res.cpu().numpy().view(np.uint32), want)
        us.sort()
        out["sizes"].append({"world": w, "n": n, "median_us": round(us[len(us) // 2], 2),
                             "p10_us": round(us[len(us) // 10], 2), "p90_us": round(us[len(us) * 9 // 10], 2)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
