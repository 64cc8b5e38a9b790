"""GPU side of the per-dataset drivers (scripts/test/test_mc1.py, test_mc3.py, test_sharad.py): the fixtures through the HIP
path, the long-list matrix-core top-k (radius 30 / 60 at 80 - 100 context frames: more than 2 048 candidates per query) against
the vector kernel and the oracle, the mc1 / mc3 drivers at their real geometry with the reference's encoder, and the command
line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, load_golden
from oracle import crw_oracle as orc
from test_segment_drivers import DRIVER_CASES, check_outputs, run_driver_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    return crw_hip


@pytest.mark.parametrize("driver", sorted(DRIVER_CASES))
def test_drivers_on_the_hip_path_match_reference_main(hip, driver):
    """The fixtures written by the reference's own main(args) through the real `utils.propagate`: every saved map exact (mc1 and
    mc3 take the long-list matrix-core top-k: 81 x 32 and 99 x 40 candidates per query), xent to 1e-4."""
    import utils as crw_utils
    g = load_golden(DRIVER_CASES[driver])
    out, n = run_driver_golden(driver, g, crw_utils.propagate, "cuda")
    assert n == int(g["n_calls"])
    check_outputs(driver, g, out)


def _layered(T, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(N + 16, C, generator=g)
    t = torch.arange(T).float()
    depth = torch.arange(N).float()[None] + 3 * torch.sin(2 * np.pi * t / 40)[:, None] + 6
    lo = depth.floor().long()
    fr = (depth - lo.float()).unsqueeze(-1)
    return (proto[lo] * (1 - fr) + proto[lo + 1] * fr + 0.3 * torch.randn(T, N, C, generator=g)).float()


@pytest.mark.parametrize("T,N,C,cxt,radius,knn,first", [
    (100, 48, 128, 80, 30, 20, 1),    # mc1 at its real geometry: 81 x 48 = 3 888 candidates
    (100, 190, 128, 100, 60, 20, 1),  # mc3 at its real geometry: 99 x 119 = 11 781
    (100, 40, 64, 100, 60, 20, 1),    # the mc3 fixture's shape: 99 x 40
    (60, 64, 128, 50, 40, 64, 1),     # 64 neighbours out of 51 x 64 = 3 264
    (100, 48, 64, 80, 30, 20, 7),     # later first frame
    (30, 300, 64, 25, 200, 10, 1)])   # a frame's band of 300 keys: three frames per chunk
def test_long_list_topk_on_matrix_cores_agrees_with_vector_kernel(hip, T, N, C, cxt, radius, knn, first):
    """Lists past 2 048 candidates (or 150 KiB of scores per tile) in chunks of context frames with the k best carried from chunk
    to chunk (labelprop_topk_mfma_kernel<CSTEPS, 0>) against the vector kernel (a 1 x N grid: the same candidates in the same
    order), with the tolerances of the two-chunk form's test, and the twin-frame exact-tie check."""
    g = torch.Generator().manual_seed(T + N + radius)
    feats = hip.normalize((torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).float().cuda())
    Wm, Im = hip.labelprop_topk(feats, cxt, radius, 0.1, knn, first_frame=first, grid_w=1)
    Wv, Iv = hip.labelprop_topk(feats, cxt, radius, 0.1, knn, first_frame=first, grid_w=N)
    torch.testing.assert_close(Wm, Wv, rtol=2e-5, atol=1e-6)
    differ = Im != Iv
    assert differ.float().mean().item() < 1e-3, f"{differ.sum().item()} of {differ.numel()} neighbours differ"
    assert (Wm[:, :-1] >= Wm[:, 1:] - 1e-7).all()
    ws = Wm.sum(1)
    torch.testing.assert_close(ws, torch.ones_like(ws), rtol=1e-5, atol=1e-5)
    feats2 = feats.clone()
    feats2[1::2] = feats2[0:T - 1:2][: feats2[1::2].shape[0]]
    Wm2, Im2 = hip.labelprop_topk(feats2, cxt, radius, 0.1, knn, first_frame=first, grid_w=1)
    Wv2, Iv2 = hip.labelprop_topk(feats2, cxt, radius, 0.1, knn, first_frame=first, grid_w=N)
    torch.testing.assert_close(Wm2, Wv2, rtol=2e-5, atol=1e-6)
    assert (Im2 != Iv2).float().mean().item() < 2e-3


@pytest.mark.parametrize("T,N,C,M,cxt,radius,temp", [(100, 48, 128, 4, 80, 30, 0.1), (100, 190, 128, 5, 100, 60, 0.01)])
def test_long_list_label_maps_match_oracle(hip, T, N, C, M, cxt, radius, temp):
    """mc1 / mc3 label-propagation settings on layered features: the label map against the fp32 oracle; a label that differs
    must be a floating-point near-tie (fp64 audit with the device's own soft labels)."""
    from imported.labelprop import LabelPropVOS_CRW
    emb = _layered(T, N, C, 77 + N)
    seed = (torch.arange(N) * M // N).float()
    ref = orc.labelprop(emb.numpy(), seed.numpy(), M, cxt, radius, temp, 20)
    feats = hip.normalize(emb.cuda())
    pred, L = LabelPropVOS_CRW(dict(CXT_SIZE=cxt, RADIUS=radius, TEMP=temp, KNN=20)).propagate_all(feats, seed.cuda(), M)
    mism = int((pred.cpu().numpy() != ref).sum())
    if mism:
        audit = orc.labelprop_tie_audit(feats.cpu().numpy(), L.cpu().numpy(), pred.cpu().numpy(), cxt, radius, temp, 20)
        assert audit["not_ties"] == 0, (mism, audit)
    assert mism <= ref.size // 100, f"{mism} of {ref.size} labels differ"


def _real_radargram(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.arange(rows).float()[:, None]
    c = torch.arange(cols).float()[None, :]
    return (torch.sin(2 * np.pi * (r + 6 * torch.sin(2 * np.pi * c / 700.0)) / 40.0) + 0.3 * torch.randn(rows, cols, generator=g))


@pytest.mark.parametrize("driver", ["mc1", "mc3"])
def test_drivers_at_real_geometry_with_the_reference_encoder(hip, driver):
    """mc1 / mc3 at their real geometry (410 rows, 32 x 32 patches, T = 100; N = 48 / 190) with a random-init Resnet in train
    mode (the scripts never call .eval()): every pass's labels are those of the same label propagation redone on the HIP features,
    and -- for radargram 0's passes -- the fp64 audit finds no label that is not a near-tie."""
    import encoder as crw_encoder
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    d = crw_inference.DRIVERS[driver]
    torch.manual_seed(11)
    enc = crw_encoder.Resnet(False).cuda()
    enc.train(True)
    rows, cols = 410, 100 * 32
    rg = [_real_radargram(rows, cols, 90 + i).cuda() for i in range(3)]
    sg = [(torch.arange(rows)[:, None] * d["nclasses"] // rows).float().repeat(1, cols).cuda() for _ in range(3)]
    sgr = [s.clone() for s in sg] if driver == "mc1" else None
    feats = {}
    hook = enc.register_forward_hook(lambda m, i, o: feats.__setitem__("emb", o.detach().clone()))
    passes = []

    def propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last):
        pred, xent, change = crw_utils.propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last)
        T, N = seq.shape[:2]
        passes.append((feats["emb"].reshape(T, N, -1).float(), crw_utils.seed_labels(seg_ref, N), pred, lp, ncls))
        return pred, xent, change

    orig = crw_inference.propagate
    crw_inference.propagate = propagate
    try:
        out = crw_inference.segment_radargrams(driver, rg, sg, enc, refs_reversed=sgr)
    finally:
        crw_inference.propagate = orig
        hook.remove()
    assert len(passes) == (6 if driver == "mc1" else 9)
    N = passes[0][0].shape[1]
    assert N == (48 if driver == "mc1" else 190)
    for k, (emb, seed, pred, lp, M) in enumerate(passes):
        ehat = hip.normalize(emb.contiguous())
        pred2, L = LabelPropVOS_CRW(dict(CXT_SIZE=lp.cxt_size, RADIUS=lp.radius, TEMP=lp.temperature, KNN=lp.topk)).propagate_all(
            ehat, seed, M)
        assert torch.equal(pred, pred2), k
        if k % 3 == 0:  # radargram 0 of every pass kind
            audit = orc.labelprop_tie_audit(ehat.cpu().numpy(), L.cpu().numpy(), pred.cpu().numpy(), lp.cxt_size, lp.radius,
                                            lp.temperature, lp.topk)
            assert audit["not_ties"] == 0, (k, audit)
    (H, _), (OH, _) = d["patch_size"], d["overlap"]
    rg_h = (N - 1) * (H - OH) + H  # the maps' rows: whole patches only (408 of 410 for mc1)
    assert list(out) == list(d["outputs"])
    for name, objs in out.items():
        if "xent" not in name:
            assert all(o.shape == (rg_h, cols) for o in objs), name


def test_cli_writes_what_the_library_computes(hip, tmp_path):
    """scripts/segment_drivers.py in a child process on a folder of the sharad driver's input files, with a saved random-init
    Resnet checkpoint (DataParallel key prefix): its output files are bit for bit those of an in-process segment_radargrams."""
    import encoder as crw_encoder
    import inference as crw_inference
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import segment_drivers as cli
    torch.manual_seed(5)
    net = crw_encoder.Resnet(False)
    torch.save({"module." + k: v for k, v in net.state_dict().items()}, tmp_path / "ck.pt")
    inp, outd = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    rows, cols = 8 * 23 + 16, 100 * 16
    for i, n in enumerate(("s_1", "s_4", "s_3")):
        torch.save(_real_radargram(rows, cols, 40 + i).half(), inp / f"{n}.pt")
        torch.save((torch.arange(rows)[:, None] * 5 // rows).repeat(1, cols).to(torch.int8), inp / f"{n}ref.pt")
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_drivers.py"), "--driver", "sharad", "--model_path",
                        str(tmp_path / "ck.pt"), "--input_folder", str(inp) + "/", "--output_folder", str(outd) + "/"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    enc = cli.load_encoder(1, str(tmp_path / "ck.pt"), "cuda")
    rg, sg, _ = cli.load_inputs("sharad", str(inp), "cuda")
    want = crw_inference.segment_radargrams("sharad", rg, sg, enc)
    assert sorted(os.listdir(outd)) == sorted(want)
    for name, objs in want.items():
        got = torch.load(outd / name, map_location="cpu")
        assert len(got) == len(objs) == 3
        for a, b in zip(got, objs):
            assert torch.equal(a.cpu(), b.cpu()), name
