"""The kernel variants behind environment switches (read once per process, so each runs in a child process): the non-default
schedules and kernels that DESIGN.md quotes A/B numbers for must stay correct, not only the defaults the rest of the suite runs."""
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

RESNET = "tests/test_resnet_hip.py"
PARITY = "tests/test_hip_parity.py"
LISTS = "tests/test_labelprop_lists_gpu.py"
GEMM_256 = "gemm_bf16 or bf16_chain_modes_on_256 or (walk_n4096 and 1-4)"
RN_PRODUCTS = "conv_forward_backward_wgrad and 128-geo1"   # P = 128 at CONVS[1] and CONVS[10..19]: every tile width, 1x1 and 3x3, strides 1 and 2
# (environment, must_run, must_not_run, test files, -k expression).  must_run / must_not_run: route names (tests/routes_ref.py) the
# child's route log (CRW_ROUTE_LOG) must / must not hold -- a switch that is shadowed, misspelled or gone runs the default kernel,
# which is correct, so the parity tests alone would pass without it.
VARIANTS = [
    # Resnet products on the all-in-one 4-wave workgroups instead of the split-role ones (csrc/resnet_gemm.hip: launch_rn_conv)
    ({"CRW_RN_SPEC": "0"}, ("rn_conv.plain_bk322",), ("rn_conv.spec2",), RESNET, "native_and_stepwise or training_step or conv_forward_backward"),
    # ... at one forced k-tile depth: CRW_RN_BK moves the plain kernel only, so it is set together with CRW_RN_SPEC=0
    ({"CRW_RN_SPEC": "0", "CRW_RN_BK": "64"}, ("rn_conv.plain_bk64",), ("rn_conv.plain_bk322", "rn_conv.spec2"), RESNET, RN_PRODUCTS),
    ({"CRW_RN_SPEC": "0", "CRW_RN_BK": "32"}, ("rn_conv.plain_bk32",), ("rn_conv.plain_bk322", "rn_conv.spec2"), RESNET, RN_PRODUCTS),
    # the split-role kernel on deeper rings, one workgroup per CU (measured slower; A/B partners)
    ({"CRW_RN_SPEC": "3"}, ("rn_conv.spec3",), ("rn_conv.spec2",), RESNET, RN_PRODUCTS),
    ({"CRW_RN_SPEC": "4"}, ("rn_conv.spec4",), ("rn_conv.spec2",), RESNET, RN_PRODUCTS),
    # 256-patch tiles on 8 waves, one workgroup per CU (measured slower; kept as the A/B partner DESIGN quotes)
    ({"CRW_RN_TM": "256"}, ("rn_conv.tm256",), (), RESNET, "native_and_stepwise or training_step or conv_forward_backward"),
    # weight gradient on 64-patch k-tiles, one workgroup per CU (the default: 32)
    ({"CRW_RN_WBK": "64"}, ("rn_wgrad.bk64",), ("rn_wgrad.bk32",), RESNET, RN_PRODUCTS),
    # BatchNorm-backward sums as a pass of their own instead of the products' LDS-staged epilogue (csrc/resnet_net.hip)
    ({"CRW_RN_FUSE_RED": "0"}, ("rn_net.bwd_separate_red",), ("rn_net.bwd_fused_red",), RESNET, "native_and_stepwise or training_step or matches_pytorch_modules"),
    # everything on the caller's stream (no side stream)
    ({"CRW_RN_STREAMS": "0"}, ("rn_net.fwd_one_stream", "rn_net.bwd_one_stream"), ("rn_net.fwd_side_stream", "rn_net.bwd_side_stream"), RESNET,
     "native_and_stepwise or training_step"),
    # forward front end on one 1024-thread workgroup per CU (csrc/encoder_front.hip)
    ({"CRW_FRONT_NT": "1024"}, ("front.fwd_nt1024",), ("front.fwd_nt512",), PARITY, "encoder_front_kernels or encoder_inference_trunk"),
    # front-end backward that ignores the saved record and recomputes conv1 / conv2 (the training path's A/B partner)
    ({"CRW_FRONT_RECOMPUTE": "1"}, ("front.bwd_recompute",), ("front.bwd_saved",), PARITY, "encoder_front_kernels_match_torch"),
    # the 3x3 layers' patch kernel forced onto 4 waves where hi/lo pairs take 8, and onto 8 where plain bf16 takes 4
    ({"CRW_CONV_NW": "4"}, ("conv.patch_nw4",), ("conv.patch_nw8",), PARITY, "encoder_conv_kernels and (3-32-64 or 3-64-128 or 3-128-128)"),
    ({"CRW_CONV_NW": "8"}, ("conv.patch_nw8",), ("conv.patch_nw4",), PARITY, "encoder_conv_kernels and (1-32-64 or 1-64-128 or 1-128-128)"),
    # the first-generation weight gradient at 128 output channels (the default there: the streamed kernel) -- the A/B partner of
    # every weight-gradient change
    ({"CRW_WGRAD": "1"}, ("wgrad.gen1",), ("wgrad.streamed",), PARITY,
     "(encoder_conv_kernels and (64-128 or 128-128)) or (wgrad_patch_slice_lengths and 3-25)"),
    # bf16 chain GEMM with its A operand staged through registers (csrc/gemm_bf16.hip)
    ({"CRW_GEMM_REGA": "1"}, ("gemm_bf16.rega",), (), PARITY, "gemm_bf16"),
    # plain-bf16 256 x 256 chain GEMM on the ring of five 32-deep half-tiles (opt-in, csrc/gemm_bf16.hip mainloop_ring5), incl. n = 4096
    ({"CRW_GEMM_RING5": "1"}, ("gemm_bf16.t256_ring5",), (), PARITY + " tests/test_k_shape.py", GEMM_256),
    # 256 x 256 chain GEMM with every wave requesting its LDS-DMA right behind the barrier (rounds 1-3; the default staggers them), and
    # with the second half of the waves requesting after a quarter of the k-tile
    ({"CRW_GEMM_STAGGER": "0"}, ("gemm_bf16.t256_stagger0",), ("gemm_bf16.t256_stagger",), PARITY + " tests/test_k_shape.py", GEMM_256),
    ({"CRW_GEMM_STAGGER": "2"}, ("gemm_bf16.t256_stagger2",), ("gemm_bf16.t256_stagger",), PARITY, "gemm_bf16"),
    # the round-3 hand-off of the sums-with-tail kernels (relaxed atomics behind s_waitcnt) and the acq_rel form: A/B partners of the
    # default release + acquire fence (csrc/resnet_bn.hip rn_sums_tail_kernel)
    ({"CRW_RN_TICKET": "relaxed"}, ("rn_bn.ticket_relaxed",), ("rn_bn.ticket_fence",), RESNET, "native_and_stepwise or training_step or reproducible"),
    ({"CRW_RN_TICKET": "acqrel"}, ("rn_bn.ticket_acqrel",), ("rn_bn.ticket_fence",), RESNET, "native_and_stepwise or reproducible"),
    # the stem's forward product at other patch sizes than 16 x 16 on the gathered product of resnet_gemm.hip where the default is the
    # band-per-wave kernel (csrc/resnet_stem.hip rn_stem_fwd_band_kernel)
    ({"CRW_RN_STEM_BAND": "0"}, ("rn_stem.gathered",), ("rn_stem.band",), RESNET,
     "matches_pytorch_modules or inference_through_propagate or training_step_matches_reference"),
    # matrix-core top-k with a query tile's scores in one piece (one workgroup per CU at config 5) where the default takes the context
    # frames in two halves through half the LDS (two workgroups per CU; csrc/labelprop.hip labelprop_topk_mfma_kernel<.., NCH>)
    ({"CRW_LABELPROP_TOPK_CHUNKS": "1"}, ("labelprop.topk_mfma_chunks1",), ("labelprop.topk_mfma_chunks2",), PARITY,
     "labelprop_topk_on_matrix_cores or labelprop_matches_oracle_mcords_shape or propagate_matches_reference"),
    # label-propagation top-k on the vector kernel where the default scores on the fp32 matrix cores (csrc/labelprop.hip)
    ({"CRW_LABELPROP_TOPK_VALU": "1"}, ("labelprop.topk_valu",),
     ("labelprop.topk_mfma_chunks1", "labelprop.topk_mfma_chunks2", "labelprop.topk_mfma_long"), PARITY,
     "labelprop_matches_oracle_mcords_shape or labelprop_edge_cases or propagate_matches_reference"),
    # crw_labelprop_propagate on the one-workgroup walk where the default chains in the role kernel + tail (A/B), against fp64
    ({"CRW_LABELPROP_GATHER_SEQ": "1"}, ("labelprop.gather_lds",), ("labelprop.propagate_prefix",), LISTS,
     "soft_labels_and_label_map_against_fp64 and (14-10-16-16-3-4-5-1 or 40-63-64-6-7-5-10-1)"),
    # the one-workgroup walk on the global-memory kernel (csrc/labelprop.hip labelprop_gather_kernel, the fallback for lists past the
    # LDS-ring form) as the thing the role kernel + tail, and the ring role kernel, are held to bit for bit: small shapes only
    ({"CRW_LABELPROP_GATHER_GLOBAL": "1"}, ("labelprop.gather_global",), ("labelprop.gather_lds",), PARITY,
     "labelprop_propagate_equals_the_one_workgroup_walk and (14-10-16-3-3-4-5-1 or 3-9-8-2-1-2-3-1 or 30-24-32-2-1-6-24-1)"),
    # (the -k words are meant to pick exactly three of test_sliding_gpu.CASES: "window of one frame", "first translated frame is the
    # last, T = cxt + 3" and "knn 4 (8 registers)"; a new case name with one of these words joins this child run)
    ({"CRW_LABELPROP_GATHER_GLOBAL": "1"}, ("labelprop.slide_general_global", "labelprop.gather_global"), ("labelprop.slide_general_lds",),
     "tests/test_sliding_gpu.py", "every_route and (window or first or (knn and 8))"),
]


def _id(row):
    return ",".join(f"{k}={v}" for k, v in row[0].items())   # (rows with the same environment: pytest numbers them)


@pytest.mark.gpu
@pytest.mark.parametrize("env,must_run,must_not_run,path,expr", VARIANTS, ids=[_id(v) for v in VARIANTS])
def test_kernel_variant_behind_env_switch(env, must_run, must_not_run, path, expr, tmp_path):
    log = tmp_path / "routes.log"
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "pytest", *[os.path.join(ROOT, p_) for p_ in path.split()], "-x", "-q", "-m", "gpu", "-k", expr,
                        "-p", "no:cacheprovider"],
                       env=dict(os.environ, CRW_ROUTE_LOG=str(log), **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
    ran = log.read_text().split() if log.exists() else []
    print(f"{env}: {time.perf_counter() - t0:.1f} s, {len(ran)} routes: {' '.join(sorted(ran))}")
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail
    assert len(set(ran)) == len(ran), "a route name is logged once per process"
    assert set(must_run) <= set(ran), (env, "the switch did not reach", sorted(set(must_run) - set(ran)), "ran", sorted(ran))
    assert not set(must_not_run) & set(ran), (env, "the default route ran beside the variant", sorted(set(must_not_run) & set(ran)))
