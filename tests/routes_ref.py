"""The route log's tables (include/crw_hip_routes.h): every name a selector passes to CRW_ROUTE, and for every CRW_* environment
switch how the suite proves that it is live.  tests/test_routes_host.py holds both against the sources; tests/test_routes_gpu.py,
tests/test_variants.py and the tests named below assert the routes of real calls."""

# every CRW_ROUTE("...") literal of csrc/, DESIGN.md section 8 has the selector and the rule of each
ROUTES = (
    # gemm_bf16.hip launch_layout
    "gemm_bf16.t128", "gemm_bf16.t256_stagger", "gemm_bf16.t256_stagger0", "gemm_bf16.t256_stagger2", "gemm_bf16.t256_ring5",
    "gemm_bf16.rega",
    # gemm_f32.hip
    "gemm_f32.t128", "gemm_f32.t64", "gemm_f32.t32", "gemm_f32.edge",
    "affinity.fwd_f32_t64", "affinity.fwd_f32_t128", "affinity.fwd_bf16x6",
    "affinity.bwd_f32_t64", "affinity.bwd_f32_t64_elem", "affinity.bwd_f32_t128_elem", "affinity.bwd_f32_t128", "affinity.bwd_bf16x6",
    # walk.hip / chain_small.hip / softmax.hip
    "walk.fwd_persistent", "walk.fwd_gemm", "walk.bwd_persistent", "walk.bwd_gemm", "chain_small.n64", "chain_small.n32",
    "softmax.stats_import", "softmax.fwd_vec", "softmax.fwd_scalar", "softmax.bwd_vec", "softmax.bwd_scalar",
    "softmax.stats_dense_vec", "softmax.stats_dense_scalar",
    # encoder_conv.hip
    "conv.patch_nw4", "conv.patch_nw8", "conv.map_big", "conv.map_small", "conv.chain", "wgrad.gen1", "wgrad.streamed", "wgrad.map",
    # encoder_front.hip
    "front.fwd_nt512", "front.fwd_nt1024", "front.bwd_saved", "front.bwd_recompute", "front.bwd_tile",
    # labelprop.hip
    "labelprop.topk_mfma_chunks1", "labelprop.topk_mfma_chunks2", "labelprop.topk_mfma_long", "labelprop.topk_valu",
    "labelprop.propagate_prefix", "labelprop.gather_lds", "labelprop.gather_global",
    "labelprop.slide_ring", "labelprop.slide_ring_origin", "labelprop.slide_general_lds", "labelprop.slide_general_global",
    "labelprop.slide_general_origin_lds", "labelprop.slide_general_origin_global",
    "labelprop.batch_reference", "labelprop.batch_slide", "labelprop.batch_slide_origin", "xent.frame", "xent.column",
    # resnet_gemm.hip / resnet_stem.hip / resnet_bn.hip / resnet_net.hip
    "rn_conv.tm256", "rn_conv.spec2", "rn_conv.spec3", "rn_conv.spec4", "rn_conv.plain_bk322", "rn_conv.plain_bk32", "rn_conv.plain_bk64",
    "rn_conv.stem_bwd_bk322", "rn_conv.stem_bwd_bk32", "rn_conv.stem_bwd_bk64", "rn_wgrad.bk32", "rn_wgrad.bk64",
    "rn_stem.patch_per_wave", "rn_stem.band", "rn_stem.gathered",
    "rn_bn.ticket_fence", "rn_bn.ticket_relaxed", "rn_bn.ticket_acqrel",
    "rn_net.fwd_side_stream", "rn_net.fwd_one_stream", "rn_net.bwd_side_stream", "rn_net.bwd_one_stream", "rn_net.bwd_fused_red",
    "rn_net.bwd_separate_red",
    # confidence.hip / labelmap_dense.hip
    "confidence.merge_vector", "confidence.merge_scalar", "dense.single", "dense.batch_chunked", "dense.batch_chunk1",
    "ordered.back_default", "ordered.back_one_word",
)

VARIANT = "variant"  # proven by a row of test_variants.VARIANTS: a child process under the switch, must_run read from CRW_ROUTE_LOG


def live(routes, proof=VARIANT):
    """the non-default value must reach `routes`; proof: VARIANT, or "tests/<file>::<test>" -- a test that sets the switch per call
    inside crw_hip.routes() and asserts them"""
    return ("routes", tuple(routes), proof)


def no_route(reason):
    return ("none", reason)


DIAG = "CRW_CONV_STAMPS-only diagnostic: the library the suite builds does not read it"
BATCHING = "host-only batching knob: splits one call into several of the same route; "

# every CRW_* name read under csrc/ and in crw_hip.py / imported/labelprop.py
SWITCHES = {
    "CRW_GEMM_REGA": live(["gemm_bf16.rega"]),
    "CRW_GEMM_RING5": live(["gemm_bf16.t256_ring5"]),
    "CRW_GEMM_STAGGER": live(["gemm_bf16.t256_stagger0", "gemm_bf16.t256_stagger2"]),
    "CRW_AFFINITY_F32": live(["affinity.fwd_f32_t128", "affinity.bwd_f32_t128"], "tests/test_routes_gpu.py::test_affinity_f32_switch_per_call"),
    "CRW_CONV_NW": live(["conv.patch_nw4", "conv.patch_nw8"]),
    "CRW_WGRAD": live(["wgrad.gen1"]),
    "CRW_CONV_CHAIN": live(["conv.patch_nw8"], "tests/test_routes_gpu.py::test_conv_chain_switch_per_call"),
    "CRW_FRONT_NT": live(["front.fwd_nt1024"]),
    "CRW_FRONT_RECOMPUTE": live(["front.bwd_recompute"]),
    "CRW_LABELPROP_TOPK_CHUNKS": live(["labelprop.topk_mfma_chunks1"]),
    "CRW_LABELPROP_TOPK_VALU": live(["labelprop.topk_valu"]),
    "CRW_LABELPROP_GATHER_GLOBAL": live(["labelprop.gather_global", "labelprop.slide_general_global"]),
    "CRW_LABELPROP_GATHER_SEQ": live(["labelprop.gather_lds"]),
    "CRW_LABELPROP_SLIDING_GENERAL": live(["labelprop.slide_general_lds", "labelprop.slide_general_origin_lds"],
                                          "tests/test_routes_gpu.py::test_sliding_ring_against_general_at_the_lds_limit"),
    "CRW_ANCHORS_RESTART_SEGMENTED": live(["labelprop.slide_ring"], "tests/test_routes_gpu.py::test_restart_segmented_switch_per_call"),
    "CRW_RN_SPEC": live(["rn_conv.plain_bk322", "rn_conv.spec3", "rn_conv.spec4"]),
    "CRW_RN_BK": live(["rn_conv.plain_bk64", "rn_conv.plain_bk32"]),
    "CRW_RN_TM": live(["rn_conv.tm256"]),
    "CRW_RN_WBK": live(["rn_wgrad.bk64"]),
    "CRW_RN_STEM_BAND": live(["rn_stem.gathered"]),
    "CRW_RN_TICKET": live(["rn_bn.ticket_relaxed", "rn_bn.ticket_acqrel"]),
    "CRW_RN_STREAMS": live(["rn_net.fwd_one_stream", "rn_net.bwd_one_stream"]),
    "CRW_RN_FUSE_RED": live(["rn_net.bwd_separate_red"]),
    "CRW_DENSE_BATCH_CHUNK": live(["dense.batch_chunk1"], "tests/test_sweep_dense_gpu.py::test_every_kernel_shape_writes_the_same_maps"),
    "CRW_ORDERED_BACK": live(["ordered.back_one_word"], "tests/test_ordered_gpu.py::test_both_backward_scans_write_the_same_maps"),
    "CRW_WGRAD_DIAG": no_route(DIAG),
    "CRW_CONV_LDS_PAD": no_route(DIAG),
    "CRW_HIP_LIB": no_route("the library path"),
    "CRW_ROUTE_LOG": no_route("the route log's own file name (tests/test_variants.py reads it back)"),
    "CRW_ANCHORS_SEGMENTED": no_route(BATCHING + "one crw_labelprop_propagate_sliding call per stretch between anchored frames "
                                      "(tests/test_anchor_lists_gpu.py holds the two arms bit for bit)"),
    "CRW_SWEEP_PER_CONFIG": no_route(BATCHING + "one propagate_all per configuration (tests/test_sweep_gpu.py, tests/test_sliding_gpu.py)"),
    "CRW_POSTERIOR_BATCH_WS": no_route(BATCHING + "the posterior batch in chunks of configurations (tests/test_sweep_posterior_gpu.py)"),
}

# routes no default-environment call may take: named by a VARIANT switch and reached under no rule of the default environment
# (conv.patch_nw4, wgrad.gen1, front.bwd_recompute, labelprop.topk_valu / gather_lds / gather_global, rn_stem.gathered and
# labelprop.topk_mfma_chunks1 are variants' routes too, but shapes reach them as well)
VARIANT_ONLY = (
    "gemm_bf16.rega", "gemm_bf16.t256_ring5", "gemm_bf16.t256_stagger0", "gemm_bf16.t256_stagger2",
    "front.fwd_nt1024", "rn_conv.plain_bk322", "rn_conv.plain_bk32", "rn_conv.plain_bk64",
    "rn_conv.spec3", "rn_conv.spec4", "rn_conv.tm256", "rn_wgrad.bk64", "rn_bn.ticket_relaxed", "rn_bn.ticket_acqrel",
    "rn_net.fwd_one_stream", "rn_net.bwd_one_stream", "rn_net.bwd_separate_red",
)
