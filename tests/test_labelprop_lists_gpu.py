"""What the label-propagation kernels WRITE -- the top-k lists (W, I, V) and the soft labels / label map (L, pred) -- against
fp64 references of the same operations (`oracle.topk_lists_audit`, `oracle.gather_audit`), over every route of
`csrc/labelprop.hip`: the vector top-k kernel, the three forms of the matrix-core top-k kernel, the prefix / tail kernels, the two
one-workgroup gather kernels and `crw_labelprop_propagate_batch`.  Every slot of every list is checked, with bounds derived from
the fp32 format next to the audits; `tests/test_labelprop_lists.py` shows on the CPU that the audits report subtly wrong lists.
Each test prints the worst observed error as a fraction of its bound, per condition."""
import pytest
import torch

from oracle import crw_oracle as orc
from test_labelprop_lists import lp_embeddings, scrambled_seed, twin_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    assert crw_hip.has_sweep()
    return crw_hip


# (T, N, C, cxt, radius, knn, first, grid_w), temperatures.  The route of each shape follows from `topk_grid` (max_nf = min(cxt + 1,
# T - 1) context frames, max_bi = min(2 radius - 1, N / grid_w) in-band rows, maxcand = max_nf * max_bi on a column):
#   matrix cores need grid_w == 1, N >= 16, C in (64, 128, 256); one launch_topk_mfma form when maxcand <= 2048 and 64 * maxcand
#   bytes <= 150 KiB -- in two halves when 64 * maxcand bytes > 76 KiB, C <= 128 and ceil(max_nf / 2) * max_bi <= 1024 --, else the
#   long-list form (C <= 128, max_bi <= 1024); everything else runs labelprop_topk_kernel.
ALL_TEMPS = (0.1, 0.01, 0.001)
TOPK_CASES = [
    ((6, 5, 7, 100, 2, 2, 1, 1), (0.1,)),         # C = 7: vector kernel, scalar dot (C % 4 != 0)
    ((10, 12, 16, 3, 2, 5, 1, 1), (0.1,)),        # N = 12 < 16, C = 16: vector kernel; truncated from frame 5; frame 1 has 3 in-band keys < knn
    ((12, 30, 16, 4, 3, 7, 1, 5), (0.1,)),        # grid_w = 5: vector kernel on a 6 x 5 grid
    ((9, 33, 20, 3, 9, 8, 2, 11), (0.1,)),        # grid_w = 11: vector kernel on a 3 x 11 grid, radius beyond the grid height, first frame 2
    ((40, 21, 64, 6, 4, 9, 1, 1), (0.1,)),        # maxcand = 7 * 7 = 49 (3 KiB): matrix cores in one piece; the second query tile has 5 of 16 nodes
    ((70, 100, 128, 9, 17, 12, 1, 1), ALL_TEMPS),  # maxcand = 10 * 33 = 330 (21 KiB): one piece; a query tile reads up to 4 key tiles
    ((30, 37, 256, 5, 1, 3, 4, 1), (0.1,)),       # maxcand = 6 * 1: one piece, 256 channels (CSTEPS = 16), the query's own node only
    ((12, 16, 128, 20, 30, 64, 1, 1), (0.1,)),    # maxcand = 11 * 16 = 176: one piece; knn = 64 > candidates up to frame 3: empty slots
    ((90, 48, 128, 80, 10, 20, 1, 1), (0.1,)),    # maxcand = 81 * 19 = 1539 <= 2048, 96 KiB > 76 KiB, 41 * 19 = 779 <= 1024: TWO HALVES (NCH = 2)
    ((100, 48, 64, 80, 30, 20, 7, 1), ALL_TEMPS),  # maxcand = 81 * 48 = 3888 > 2048: long-list form (NCH = 0), 4 chunks of 21 frames, first frame 7
    ((60, 64, 128, 50, 40, 64, 1, 1), (0.1,)),    # maxcand = 51 * 64 = 3264 > 2048: long-list form, 4 chunks of 13 frames, knn = 64
]


def _report(what, res):
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in res["worst"].items()))
    assert not any(res["violations"].values()), (what, res)
    assert all(v <= 1 for v in res["worst"].values()), (what, res)


@pytest.mark.parametrize("shape,temp", [(s, t) for s, temps in TOPK_CASES for t in temps],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_topk_lists_against_fp64(hip, shape, temp):
    T, N, C, cxt, radius, knn, first, gw = shape
    feats = hip.normalize(lp_embeddings(T, N, C, T + N).cuda())
    for name, f in (("plain", feats), ("twin frames", twin_frames(feats).contiguous())):
        W, I = hip.labelprop_topk(f, cxt, radius, temp, knn, first_frame=first, grid_w=gw)
        V, Iv = hip.labelprop_topk_scores(f, cxt, radius, temp, knn, first_frame=first, grid_w=gw)
        assert torch.equal(I, Iv), "the scores mode selects other candidates than the weights mode"
        res = orc.topk_lists_audit(f, cxt, radius, temp, knn, first, gw, W, I, V)
        if name == "twin frames":   # the tie rule is exercised: neighbouring slots with the same logit bit for bit
            full = V[:, 1:] != -float("inf")
            assert bool(((V[:, :-1] == V[:, 1:]) & full).any())
        _report(f"{shape} temp {temp} {name}", res)


# (T, N, C, M, cxt, radius, knn, grid_w): the lists of one shape per route of test_labelprop_propagate_equals_the_one_workgroup_walk,
# with a scrambled seed.  crw_labelprop_propagate chains the frames 1 .. cxt in labelprop_prefix_kernel<8 / 16 / 24> when knn <= 24 and
# the N * M outputs of a frame fit 6 compute waves (N * M <= 384; M is chosen to stay below that where the prefix kernel is meant),
# and runs every later frame in labelprop_tail_batch_kernel (one configuration); otherwise it calls crw_labelprop_gather, which takes labelprop_gather_lds_kernel
# when knn * N <= 2048 and at least 4 frames fit its LDS ring, else labelprop_gather_kernel.  crw_labelprop_propagate_batch always
# runs labelprop_chain_batch_kernel + labelprop_tail_batch_kernel.
GATHER_CASES = [
    (14, 10, 16, 16, 3, 4, 5, 1),     # knn 5: prefix<8> (160 outputs: 3 compute waves) for frames 1 .. 3, tail for 4 .. 13
    (40, 63, 64, 6, 7, 5, 10, 1),     # knn 10: prefix<16> (378 outputs: 6 compute waves, M = 6 keeps it there) for frames 1 .. 7, tail
    (30, 24, 32, 16, 1, 6, 24, 1),    # knn 24: prefix<24> (384 outputs) for frame 1 alone, tail for 2 .. 29
    (20, 120, 32, 16, 3, 4, 6, 1),    # 1920 outputs per frame (600 and more: beyond the compute waves): the LDS-ring one-workgroup kernel
    (16, 40, 32, 16, 5, 40, 30, 1),   # 30 neighbours > 24: the LDS-ring one-workgroup kernel (knn * N = 1200 <= 2048)
    (12, 30, 16, 3, 4, 3, 7, 5),      # 6 x 5 grid, M = 3: prefix<8> for frames 1 .. 4, tail
    (2, 10, 16, 16, 3, 4, 5, 1),      # T = 2: no chained frame, the seed path of the one-workgroup kernel
    (8, 70, 32, 16, 3, 40, 30, 1),    # knn * N = 2100 > 2048 = GATHER_NT * GATHER_PF: labelprop_gather_kernel, the global one, from both entry points
]


def _gather_report(what, res):
    print(f"{what}: worst error / bound soft {res['worst']['soft']:.3g} (bound {res['bound']:.3g})")
    assert not any(res["violations"].values()), (what, res)


@pytest.mark.parametrize("T,N,C,M,cxt,radius,knn,grid_w", GATHER_CASES)
def test_soft_labels_and_label_map_against_fp64(hip, T, N, C, M, cxt, radius, knn, grid_w):
    feats = hip.normalize(lp_embeddings(T, N, C, T * 7 + N).cuda())
    seed = scrambled_seed(N, M).cuda()
    assert bool((seed[1:] != seed[:-1]).all())
    W, I = hip.labelprop_topk(feats, cxt, radius, 0.1, knn, first_frame=1, grid_w=grid_w)
    W2, I2 = hip.labelprop_topk(feats, cxt, radius, 0.05, knn, first_frame=1, grid_w=grid_w)   # the batch's second configuration
    lists = [(W, I), (W2, I2)]
    tag = f"{(T, N, C, M, cxt, radius, knn, grid_w)}"
    L0, p0 = hip.labelprop_gather(seed, W, I, T, N, M, first_frame=1)
    _gather_report(f"{tag} gather", orc.gather_audit(W, I, seed, M, 1, cxt, L0, p0))
    L1, p1 = hip.labelprop_gather(seed, W, I, T, N, M, first_frame=1, cxt_size=cxt)
    _gather_report(f"{tag} propagate", orc.gather_audit(W, I, seed, M, 1, cxt, L1, p1))
    Lb, pb = hip.labelprop_propagate_batch(seed, torch.stack([W, W2]), torch.stack([I, I2]), T, N, M, first_frame=1, cxt_size=cxt)
    for g, (Wg, Ig) in enumerate(lists):
        _gather_report(f"{tag} propagate_batch[{g}]", orc.gather_audit(Wg, Ig, seed, M, 1, cxt, Lb[g], pb[g]))
    if T == 2:
        return
    # a later first frame, the earlier labels given: frames before it stay as they were, the rest as above
    first = 2
    L_init, p_init = L0.clone(), torch.full((N, T), -1.0).cuda()
    L_init[first * N:] = -7.0
    Wf, If = W[first - 1:].contiguous(), I[first - 1:].contiguous()
    for name, kw in (("gather", {}), ("propagate", dict(cxt_size=cxt))):
        La, pa = L_init.clone(), p_init.clone()
        hip.labelprop_gather(None, Wf, If, T, N, M, first_frame=first, L=La, pred=pa, **kw)
        _gather_report(f"{tag} {name} from frame {first}", orc.gather_audit(Wf, If, seed, M, first, cxt, La, pa, L_init, p_init))
    Lg, pg = torch.stack([L_init, L_init]), torch.stack([p_init, p_init])
    hip.labelprop_propagate_batch(None, torch.stack([Wf, W2[first - 1:]]), torch.stack([If, I2[first - 1:]]), T, N, M, first_frame=first,
                                  cxt_size=cxt, L=Lg, pred=pg)
    for g, (Wg, Ig) in enumerate(lists):
        _gather_report(f"{tag} propagate_batch[{g}] from frame {first}",
                       orc.gather_audit(Wg[first - 1:], Ig[first - 1:], seed, M, first, cxt, Lg[g], pg[g], L_init, p_init))
