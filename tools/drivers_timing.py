"""Per-call times of the label-propagation top-k at the mc1 / mc3 settings, the propagation at mc3's node count, and whole
driver runs (3 radargrams, all passes) at real geometry with a random-init Resnet in train mode.  argv[1]: 'topk' | 'drivers' | 'pass' (one mc1 and one mc3 forward pass, for rocprofv3).
usage: python tools/drivers_timing.py topk   (CRW_LABELPROP_TOPK_VALU=1 for the vector kernel)"""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd")]
import numpy as np
import torch
import crw_hip

def ev_time(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps

mode = sys.argv[1]
res = {"mode": mode, "valu": os.environ.get("CRW_LABELPROP_TOPK_VALU", "0")}
if mode == "topk":
    for name, (T, N, C, cxt, r, temp, M) in {"mc1": (100, 48, 128, 80, 30, 0.1, 4), "mc3": (100, 190, 128, 100, 60, 0.01, 5)}.items():
        g = torch.Generator().manual_seed(1)
        feats = crw_hip.normalize((torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).float().cuda())
        res[f"{name}_topk_ms"] = ev_time(lambda: crw_hip.labelprop_topk(feats, cxt, r, temp, 20))
        W, I = crw_hip.labelprop_topk(feats, cxt, r, temp, 20)
        seed = (torch.arange(N) * M // N).float().cuda()
        res[f"{name}_propagate_ms"] = ev_time(lambda: crw_hip.labelprop_gather(seed, W, I, T, N, M, cxt_size=cxt), reps=5, warm=1)
elif mode in ("drivers", "pass"):
    import encoder as crw_encoder, inference as crw_inference, utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    torch.manual_seed(11)
    enc = crw_encoder.Resnet(False).cuda()
    enc.train(True)
    rows, cols = 410, 3200
    g = torch.Generator().manual_seed(3)
    r = torch.arange(rows).float()[:, None]; c = torch.arange(cols).float()[None, :]
    rg = [(torch.sin(2 * np.pi * (r + 6 * torch.sin(2 * np.pi * c / 700.0)) / 40.0) + 0.3 * torch.randn(rows, cols, generator=g)).cuda() for _ in range(3)]
    for drv in ("mc1", "mc3"):
        d = crw_inference.DRIVERS[drv]
        sg = [(torch.arange(rows)[:, None] * d["nclasses"] // rows).float().repeat(1, cols).cuda() for _ in range(3)]
        if mode == "pass":  # one forward pass of radargram 0 (after one warm-up pass), for the kernel listing
            items = crw_inference._items(rg[0], d["patch_size"], d["overlap"])
            lp = LabelPropVOS_CRW(dict(CXT_SIZE=d["cxt_size"], RADIUS=d["radius"], TEMP=d["temp"], KNN=d["knn"]))
            for _ in range(2):
                crw_utils.propagate(items, sg[0][:, :32], enc, lp, d["nclasses"], False, False)
            torch.cuda.synchronize()
            continue
        run = lambda: crw_inference.segment_radargrams(drv, rg, sg, enc, refs_reversed=sg if drv == "mc1" else None)
        run(); torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        res[f"{drv}_driver_ms"] = sorted(ts)[1]
        res[f"{drv}_driver_ms_all"] = ts
print(json.dumps(res))
