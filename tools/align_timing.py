"""What aligning a bank to its item costs: the entry points of include/crw_hip_align.h against the ones they stand beside, and the
existing top-k entry points of this build against a build of the parent commit -- at tools/sliding_timing.py's geometries (cfg5
[T, N] = [256, 48] and an mc1-like item [100, 48], CXT_SIZE 80, KNN 20, RADIUS 10, C 128), a bank of four traces (n_long = 5 with
the item's seed frame, first_frame = 5), by tools/longmem_timing.py's protocol.  Centring (the (4 + T) * N rows of bank and item):

  nz            crw_normalize on those rows
  cn / cnd      crw_center_normalize, two segments (the bank's 4 * N rows, the item's T * N), the offsets by value / on the device
  pt            the PyTorch-ROCm composite on the same two segments: mean(0), subtract, F.normalize (fp32 throughout)

top-k lists:

  tl / tg       crw_labelprop_topk_long (n_long 5) / crw_labelprop_topk_grid, this build
  tl0 / tg0     the same calls on the library given by --parent_lib (built from the parent commit), loaded by path beside this
                build's.  Left out when no such library is given.  Known artefact of this way of measuring: the library loaded
                second tends to run about 1 % faster
  tb0 / tb1     crw_labelprop_topk_long_bias at long_bias 0 (which runs tl's kernels: the same bits, asserted) and 0.1

Buffers allocated once, 20 calls per round between two device events, seven rounds alternating the arms after a warm-up of each;
every round is on the log line.  --segment: `inference.segment(memory=4 traces)` without and with memory_align='center',
memory_bias=0.1 on --synthetic 410 8192 with the CNN, alternating, wall clock around a synchronised call, seven rounds.

usage: python tools/align_timing.py [--parent_lib FILE] [--segment] [--out FILE]
One JSON line per geometry, appended to FILE (default profiles/align_timing.log) and printed."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from sliding_timing import C, GEOM, RADIUS, ROUNDS, TEMP, alternate, checked, emit, stats

BANK, BIAS = 4, 0.1


def parent_entries(path):
    """crw_labelprop_topk_long and crw_labelprop_topk_grid of another build of the library, loaded by path"""
    handle = ctypes.CDLL(path)
    handle.crw_abi_version.restype = ctypes.c_int
    assert handle.crw_abi_version() == crw_hip.ABI_VERSION
    out = []
    for name, table in (("crw_labelprop_topk_long", crw_hip.LONGMEM_SIGNATURES), ("crw_labelprop_topk_grid", crw_hip.SIGNATURES)):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = table[name]
        out.append(fn)
    return out


def run(out, parent_lib):
    lib = crw_hip.lib()
    parent = parent_entries(parent_lib) if parent_lib else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    for name, g in GEOM.items():
        T, N, cxt, knn = g["T"], g["N"], g["cxt"], g["knn"]
        F, K = BANK + T, BANK + 1
        rows = F * N
        gen = torch.Generator().manual_seed(1)
        emb = (torch.randn(1, N, C, generator=gen) + 0.5 * torch.randn(F, N, C, generator=gen) + torch.randn(C, generator=gen)).float().cuda()
        emb[:BANK] += torch.randn(C, generator=gen).cuda()            # the bank a class distance away from the item
        flat = emb.reshape(rows, C)
        bounds = [0, BANK * N, rows]
        seg_host, seg_dev = (ctypes.c_int32 * 3)(*bounds), torch.tensor(bounds, dtype=torch.int32, device="cuda")
        nbytes = lib.crw_center_normalize_ws_bytes(rows, C, 2)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        e_nz, e_cn, e_cnd = (torch.empty(rows, C, device="cuda") for _ in range(3))
        center_arms = dict(
            nz=lambda: checked(lib.crw_normalize(p(flat), rows, C, p(e_nz), None, None), "normalize"),
            cn=lambda: checked(lib.crw_center_normalize(p(flat), rows, C, None, seg_host, 2, p(ws), nbytes, p(e_cn), None, None), "center"),
            cnd=lambda: checked(lib.crw_center_normalize(p(flat), rows, C, p(seg_dev), None, 2, p(ws), nbytes, p(e_cnd), None, None), "center"))

        def arm_pt():
            a, b = flat[:BANK * N], flat[BANK * N:]
            return torch.cat([torch.nn.functional.normalize(a - a.mean(0), dim=-1), torch.nn.functional.normalize(b - b.mean(0), dim=-1)])

        center_arms["pt"] = arm_pt
        for fn in center_arms.values():
            fn()
        torch.cuda.synchronize()
        assert bits(e_cn, e_cnd), "cn and cnd differ"
        pt_err = float((arm_pt() - e_cn).abs().max())
        feats = e_cn.reshape(F, N, C)
        lists = lambda ff: (torch.empty(F - ff, knn, N, device="cuda"), torch.empty(F - ff, knn, N, device="cuda", dtype=torch.int32))
        (Wl, Il), (Wl0, Il0), (Wb0, Ib0), (Wb1, Ib1), (Wg, Ig), (Wg0, Ig0) = lists(K), lists(K), lists(K), lists(K), lists(1), lists(1)
        long_ = lambda fn, W, I: checked(fn(p(feats), F, N, C, cxt, K, RADIUS, TEMP, knn, K, p(W), p(I), 0, 0, None), "topk_long")
        grid = lambda fn, W, I: checked(fn(p(feats), F, N, C, cxt, RADIUS, TEMP, knn, 1, 1, p(W), p(I), None), "topk_grid")
        bias = lambda b, W, I: checked(lib.crw_labelprop_topk_long_bias(p(feats), F, N, C, cxt, K, RADIUS, TEMP, knn, K, p(W), p(I), 0, 0, b, None),
                                       "topk_long_bias")
        arms = dict(tl=lambda: long_(lib.crw_labelprop_topk_long, Wl, Il), tg=lambda: grid(lib.crw_labelprop_topk_grid, Wg, Ig))
        if parent is not None:
            arms.update(tl0=lambda: long_(parent[0], Wl0, Il0), tg0=lambda: grid(parent[1], Wg0, Ig0))
        arms.update(tb0=lambda: bias(0.0, Wb0, Ib0), tb1=lambda: bias(BIAS, Wb1, Ib1))
        with crw_hip.routes() as hit:
            for k in ("tl", "tg", "tb0", "tb1"):
                arms[k]()
        if parent is not None:
            arms["tl0"](), arms["tg0"]()
        torch.cuda.synchronize()
        assert bits(Wl, Wb0) and torch.equal(Il, Ib0), "a zero bias and topk_long differ"
        if parent is not None:
            assert bits(Wl, Wl0) and torch.equal(Il, Il0) and bits(Wg, Wg0) and torch.equal(Ig, Ig0), "this build and the parent differ"
        arms.update(center_arms)   # the top-k arms first: the composite allocates, and the arm behind it pays for that
        res = alternate(arms)
        med = lambda k: stats(res[k])["median"]
        extra = dict(cn_over_nz=med("cn") / med("nz"), cnd_over_cn=med("cnd") / med("cn"), cn_over_pt=med("cn") / med("pt"),
                     tb0_over_tl=med("tb0") / med("tl"), tb1_over_tl=med("tb1") / med("tl"),
                     slots_moved_by_the_bias=int((Ib1 != Il).sum()), slots=Il.numel())
        if parent is not None:
            for k in ("tl", "tg"):
                s0 = stats(res[k + "0"])
                extra[k + "_median_within_parent_rounds"] = bool(s0["min"] <= med(k) <= s0["max"])
                extra[k + "_over_parent"] = med(k) / s0["median"]
            for k in ("tb0", "tb1"):
                extra[k + "_over_parent_tl"] = med(k) / med("tl0")
        emit(out, what="align", geom=name, unit="us per call", T=T, N=N, cxt=cxt, knn=knn, radius=RADIUS, C=C, bank=BANK, n_long=K, rows=rows,
             bias=BIAS, parent_lib=bool(parent), routes=sorted(hit), composite_max_abs_diff=pt_err, rounds=res,
             **{k + "_stats": stats(v) for k, v in res.items()}, tl_tb0_bitwise_equal=True, **extra)


def segment(out):
    """`segment(memory=4 traces)` against the same with memory_align='center', memory_bias=0.1 on --synthetic 410 8192
    (segment_all.py's defaults, the CNN, CONTEXT sliding)"""
    import inference
    import utils
    from imported.labelprop import LabelPropVOS_CRW
    sys.path.insert(0, os.path.join(ROOT, "radar-sounder-crw_amd", "scripts"))
    import segment_all
    args = segment_all.with_defaults(segment_all.get_args_parser().parse_args(["--synthetic", "410", "8192", "--context", "sliding"]))
    torch.manual_seed(11)
    enc = utils.create_model(args.model, args.pos_embed).cuda()
    dataset, nclasses, seg, _ = segment_all.load_data(args)
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=args.cxt_size, RADIUS=args.radius, TEMP=args.temp, KNN=args.knn, CONTEXT="sliding"))
    T, (W, ow) = args.seq_length, (args.patch_size[1], args.overlap[1])
    rg_len = T * (W - ow) + ow
    bank = utils.bank_from_columns(dataset, seg.cpu(), [0, rg_len // 3, 2 * rg_len // 3, rg_len - W])
    call = lambda **kw: inference.segment(dataset, seg, enc, lp, nclasses, T, args.patch_size, args.overlap, dataset_id=args.dataset, memory=bank, **kw)
    arms = dict(memory=lambda: call(), center=lambda: call(memory_align="center"), bias=lambda: call(memory_bias=BIAS),
                both=lambda: call(memory_align="center", memory_bias=BIAS))
    res = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[k].append(round((time.perf_counter() - t0) * 1e3, 2))
    m = stats(res["memory"])["median"]
    emit(out, what="segment with a bank of 4 traces: the two options", synthetic=[410, 8192], unit="ms per call", seq_length=T,
         patch_size=list(args.patch_size), cxt=args.cxt_size, knn=args.knn, radius=args.radius, radargrams=seg.shape[-1] // rg_len, rounds=res,
         **{k + "_stats": stats(v) for k, v in res.items()}, **{k + "_over_memory": stats(res[k])["median"] / m for k in ("center", "bias", "both")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.log"))
    ap.add_argument("--parent_lib", default=None, help="a libcrw_hip.so built from the parent commit (arms tl0, tg0)")
    ap.add_argument("--segment", action="store_true", help="also time segment(memory=) without and with the two options")
    a = ap.parse_args()
    run(a.out, a.parent_lib)
    if a.segment:
        segment(a.out)


if __name__ == "__main__":
    main()
