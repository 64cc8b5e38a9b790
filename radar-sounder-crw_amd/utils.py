"""Factories and inference glue with the reference's names and signatures (src/utils.py):
``create_model``, ``create_dataset``, ``get_reference``, ``pos_embed``, ``propagate``,
``ndiag_matrix``.  Device-agnostic where the reference hard-codes ``'cuda'``.
"""
import os

import torch
import torch.nn.functional as TF
from torch.utils.data import Subset

import crw_hip
from encoder import CNN, Resnet
from dataset import RGDataset, trim_miguel, synthetic_radargram

# dataset id -> (radargram path, reference-segmentation path, number of classes); the reference
# hard-codes these (src/utils.py:30-38, 57-70).  CRW_DATA_ROOT re-roots them.
_DATA = {
    0: ('/data/MCoRDS1_2010_DC8/RG2_MCoRDS1_2010_DC8.pt', '/data/MCoRDS1_2010_DC8/SG2_MCoRDS1_2010_DC8.pt', 4),
    1: ('/datasets/MCORDS1_Miguel/rg2.pt', '/datasets/MCORDS1_Miguel/seg3.pt', 6),
    2: (None, '/data/MCoRDS1_2010_DC8/SG3_MCoRDS1_2010_DC8.pt', 4),
    3: ('/datasets/SHARAD/sharad_north_rg.pt', '/datasets/SHARAD/sharad_north_sg5.pt', 5),
}


def _rooted(path):
    root = os.environ.get('CRW_DATA_ROOT')
    return os.path.join(root, path.lstrip('/')) if root else path


def create_model(id, pos_embed):
    if id == 0:
        return CNN(pos_embed)
    if id == 1:
        return Resnet(pos_embed)
    raise ValueError(f'unknown model id {id} (0 = CNN, 1 = Resnet)')


def create_dataset(id, length, dim, overlap, full=False, flip=False, data_path=None, synthetic=None):
    """id 0/1/3 = MCoRDS1 / MCoRDS3 / SHARAD at the reference's paths.  Extensions: ``data_path``
    (any H x W ``.pt`` radargram) and ``synthetic=(H, W)`` (seeded generator, no file)."""
    if synthetic is not None:
        ds = RGDataset.synthetic(synthetic[0], synthetic[1], length, dim, overlap)
    else:
        path = data_path if data_path is not None else _rooted(_DATA[id][0])
        ds = RGDataset(filepath=path, length=length, dim=dim, overlap=overlap, flip=flip)
    if full:
        return ds
    print('Non-Overlapping dataset! Number of items is the above divided by the length of the sequence...')
    return Subset(ds, range(0, len(ds), length))


def get_reference(id, h, w, flip=False, length=None, dim=None, overlap=None, seg_path=None):
    """-> (nclasses, reference segmentation [h, w or full width]) for dataset ``id``."""
    _, path, nclasses = _DATA[id]
    data = torch.load(seg_path if seg_path is not None else _rooted(path))
    if id == 1:
        data = trim_miguel(data, length, dim)
    data = data[:h, :] if w == 0 else data[:h, :w]
    return (nclasses, torch.flip(data, (1,))) if flip else (nclasses, data)


def pos_embed(seq):
    """[P,1,H,W] -> [P,2,H,W]: prepends a channel holding the row position r/H - 0.5."""
    P, _, H, W = seq.shape
    pe = (torch.arange(H, device=seq.device, dtype=torch.float32) / H - 0.5).view(1, 1, H, 1)
    return torch.cat([pe.expand(P, 1, H, W).to(seq.dtype), seq], dim=1)


def seed_labels(seg_ref, N):
    """Nearest-neighbour resize of the reference segmentation [rows, w] to one label per node
    (torchvision Resize((N,1), NEAREST) in the reference, src/utils.py:139-141)."""
    return TF.interpolate(seg_ref[None, None].float(), size=(N, 1), mode='nearest')[0, 0, :, 0]


def anchor_nodes(annot, cols, rg_len, T, N, rg_h, step_w):
    """Annotated pixel columns -> node anchors (CPU): one [T, N] int8 tensor per radargram, in the ITEM's frame order, -1 = free --
    what `propagate(anchors=)` takes.  annot [rows, width] integer labels (< 0 = unlabelled), cols: the annotated pixel columns;
    rg_len pixel columns per radargram, step_w = W - ow columns between the starts of two frames, rg_h the rows the N nodes span.
    Pixel column x belongs to radargram x // rg_len and to frame min((x mod rg_len) // step_w, T - 1); its node labels are
    annot[floor(n * rg_h / N), x], the row rule of `seed_labels`.  Two annotated columns in one frame: the later column wins."""
    annot = torch.as_tensor(annot).cpu()
    n_rg = annot.shape[-1] // rg_len
    out = [torch.full((T, N), -1, dtype=torch.int8) for _ in range(n_rg)]
    xs = sorted(int(c) for c in cols)
    if xs and not 0 <= xs[0] <= xs[-1] < n_rg * rg_len:
        raise ValueError(f"annotated columns {xs[0]} .. {xs[-1]} lie outside the {n_rg} radargram(s) of {rg_len} columns")
    node_rows = torch.div(torch.arange(N) * rg_h, N, rounding_mode='floor')
    vals = annot[node_rows][:, xs].to(torch.int64)                                   # [N, len(xs)]
    if vals.numel() and int(vals.max()) > 127:
        raise ValueError(f"the annotated columns hold class {int(vals.max())}: anchors are int8")
    vals = torch.where(vals >= 0, vals, torch.full_like(vals, -1)).to(torch.int8)
    for k, x in enumerate(xs):                                                       # ascending: the later column wins
        out[x // rg_len][min((x % rg_len) // step_w, T - 1)] = vals[:, k]
    return out


class MemoryBank(object):
    """Fully labelled traces from elsewhere -- another item, another radargram -- for `propagate(memory=)`: patches [B, N, h, w]
    float32 (a trace is one patch column, what a frame of an item is) and labels [B, N] int8, one class per node.  `memory_bank`
    makes one from tensors, `bank_from_columns` cuts one out of an annotated dataset; `save` / `load` keep it in an .npz file."""

    def __init__(self, patches, labels):
        self.patches, self.labels = patches, labels

    def __len__(self):
        return self.patches.shape[0]

    @property
    def nodes(self):
        return self.patches.shape[1]

    def save(self, path):
        import numpy as np
        np.savez(path, patches=self.patches.cpu().numpy(), labels=self.labels.cpu().numpy())

    @staticmethod
    def load(path):
        import numpy as np
        g = np.load(path)
        return memory_bank(torch.from_numpy(g["patches"]), torch.from_numpy(g["labels"]))


def memory_bank(traces, labels):
    """traces [B, N, h, w] (patch columns as `dataset` cuts them), labels [B, N] int8 -> MemoryBank.  Fully labelled traces only:
    a negative label is refused (partially labelled traces belong inside their item, as anchors)."""
    traces, labels = torch.as_tensor(traces), torch.as_tensor(labels)
    if traces.dim() != 4 or traces.shape[0] < 1 or labels.dtype != torch.int8 or tuple(labels.shape) != tuple(traces.shape[:2]):
        raise ValueError(f"a memory bank is traces [B >= 1, N, h, w] and labels [B, N] int8 (got {tuple(traces.shape)}, "
                         f"{labels.dtype} {tuple(labels.shape)})")
    if bool((labels < 0).any()):
        raise ValueError("a memory bank holds fully labelled traces only: every node needs a class >= 0")
    return MemoryBank(traces.float().contiguous(), labels.contiguous())


def bank_from_columns(dataset, annot, cols):
    """The bank of the patch columns that START at the pixel columns `cols` of an RGDataset's radargram (a start is clipped so that
    the column of patches fits the width), cut as the dataset cuts its frames and labelled from annot [rows, width] at the start
    column itself by the row rule of `seed_labels`: node n takes annot[floor(n * rg_h / N), x], rg_h the rows the N nodes span."""
    image, annot = dataset.T, torch.as_tensor(annot)
    h, w, oh, N, rg_h = dataset.h, dataset.w, dataset.oh, dataset.nh, dataset.nh * (dataset.h - dataset.oh) + dataset.oh
    width = min(image.shape[-1], annot.shape[-1])
    xs = [min(max(int(c), 0), width - w) for c in cols]
    if not xs:
        raise ValueError("a memory bank needs at least one column")
    traces = torch.stack([torch.stack([image[n * (h - oh):n * (h - oh) + h, x:x + w] for n in range(N)]) for x in xs])
    node_rows = torch.div(torch.arange(N) * rg_h, N, rounding_mode='floor')
    vals = annot[node_rows][:, xs].to(torch.int64).t()
    if int(vals.max()) > 127:
        raise ValueError(f"the annotated columns hold class {int(vals.max())}: bank labels are int8")
    return memory_bank(traces, vals.to(torch.int8))


def column_diffs_async(xent):
    """|xent[:, i] - xent[:, i+1]| summed over the nodes (src/utils.py:125), copied to pinned host memory WITHOUT
    blocking: -> (host tensor, event).  Lets the caller queue more GPU work before the host needs the values."""
    d = (xent[:, :-1] - xent[:, 1:]).abs().sum(0)
    host = torch.empty(d.shape, dtype=d.dtype, pin_memory=True)
    host.copy_(d, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return host, ev


def change_point(xent, diffs=None):
    """PELT(rbf, pen=5) on the column-to-column change of the metric, then `result[-2] + 5` clamped at 0
    (src/utils.py:125-132).  Uses `ruptures` when it is importable, else the restatement of its published
    algorithm in pelt.py (parity unpinned, see there); like the reference, any failure -- e.g. fewer than
    two breakpoints -- yields None.  (`crw_hip.pelt_rbf` is pelt.py's arithmetic as a host function of the library: the numpy
    form took 0.9 ms per radargram and had become the tail of the config-5 step.)  diffs: the (host, event) pair of `column_diffs_async` if already requested."""
    if diffs is not None:
        diffs[1].synchronize()
        diffs = diffs[0].numpy()
    else:
        diffs = (xent[:, :-1] - xent[:, 1:]).abs().sum(0).cpu().numpy()
    try:
        try:
            import ruptures as rpt
            result = rpt.Pelt(model="rbf").fit(diffs).predict(pen=5)
        except ImportError:  # pelt.py's restatement, as the library's host function (csrc/pelt.cpp: same sums, plain C++)
            result = crw_hip.pelt_rbf(diffs, pen=5)
        return max(0, int(result[-2] + 5))
    except Exception:
        return None


def _features_and_seed(seq, seg_ref, model, do_pos_embed, use_last, memory=None, memory_align=None):
    """The front of `propagate` / `propagate_sweep`: ONE encoder call on the whole item (the batch matters for the `Resnet`, whose
    train-mode BatchNorm statistics are the batch's), normalised features [T,N,C] and the seed labels [N].
    memory (a MemoryBank): its B * N patches go through the SAME encoder call, in front of the item's -- one BatchNorm batch in
    train mode -- and the result gains the bank's features [B,N,C]; seg_ref None: no seed (None).
    memory_align 'center' (with a bank): the raw features are two segments, the bank's B * N rows and the item's T * N rows; each is
    centred by its own per-channel mean before the normalisation (`crw_hip.center_normalize`, crw_center_normalize)."""
    T, N, H, W = seq.shape
    if memory is None and seg_ref is None:
        raise ValueError("seg_ref=None (no seed) needs memory: without a bank nothing labels the item's first frame")
    if use_last:
        seq = torch.flip(seq, (0,))
    B = 0 if memory is None else len(memory)
    if B:
        seq = torch.cat([memory.patches.to(device=seq.device, dtype=seq.dtype), seq])
    x = seq.reshape(-1, H, W).unsqueeze(1)
    if do_pos_embed:
        x = pos_embed(x)
    emb = model(x).reshape(B + T, N, -1).float().contiguous()
    if B and memory_align == 'center':
        feats = crw_hip.center_normalize(emb, [0, B * N, (B + T) * N])
    else:
        feats = crw_hip.normalize(emb)
    if memory is None:
        return feats, seed_labels(seg_ref.to(feats.device), N)
    return feats[B:], (None if seg_ref is None else seed_labels(seg_ref.to(feats.device), N)), feats[:B]


@torch.no_grad()
def propagate(seq, seg_ref, model, lp, nclasses, do_pos_embed, use_last, *, confidence=None, soft=False, anchors=None,
              anchor_context='clamp', novelty=False, novelty_top=None, memory=None, memory_align=None, memory_bias=0.0):
    """seq [T,N,h,w]; seg_ref [rows, w] class ids of the first (or last) frame; model: encoder;
    lp: LabelPropVOS_CRW  ->  (labels [N,T] float, xent [N,T-1] (CPU), change_idx | None).

    anchors: None, or [T, N] int8 in the ITEM's frame order (`anchor_nodes`; flipped along T with ``seq`` under ``use_last``):
    labelled nodes inside the item, handed to ``lp.propagate_all`` (which needs CONTEXT 'sliding'); the row of the pass's seed frame
    is ignored.  A one-frame item ignores them.
    anchor_context: 'clamp', or 'restart' (needs anchors): ``lp.propagate_all``'s option -- the context restarts at every fully
    anchored frame, in the pass's own frame order (under ``use_last`` on the mirrored anchors).

    confidence: None, or a kind of `crw_hip.labelprop_confidence` ('maxprob', 'margin', 'entropy') -- the tuple then gains a
    fourth entry, conf [N,T] float on the labels' device: the confidence of every label, from the soft labels the propagation
    wrote (the reference arg-maxes them away, src/utils.py:160); 1 in the seed column.  The labels do not depend on it.
    soft: the tuple gains, as its LAST entry, the soft labels themselves: L [T*N, M] float32 on the labels' device, node (n, t) in
    row t*N + n, frames in the pass's own order (reversed under ``use_last``, like the labels); frame 0 -- and a one-frame item --
    is the one-hot of the seed.  What `crw_hip.labelmap_dense` turns into a pixel map.
    novelty: the tuple gains one entry, behind conf when that is present and before L: (nov [N,T], score [T]) float32 on the labels'
    device, frames in the pass's own order -- `lp.novelty` on the SAME features (the encoder does not run again), under the pass's
    anchors and anchor_context; column / entry 0 (the seed frame has no keys) is 0.  novelty_top: how many of a frame's largest
    node novelties its score averages (None: max(1, N // 4)).  What `crw_hip.suggest_frames` reads.  The labels do not depend on
    it.
    memory: None, or a `MemoryBank` of B fully labelled traces from elsewhere (needs CONTEXT 'sliding', anchor_context 'clamp', no
    novelty): its patches are encoded in the same encoder call as the item and stand in front of it as long-term frames
    (``lp.propagate_all(memory=)``).  With a bank ``seg_ref`` may be None: the item has no seed, its first frame is predicted from
    the bank alone and its confidence is that of any other frame.  Everything returned is the item's, as without a bank.
    memory_align (needs memory): None, or 'center' -- the bank's features and the item's are each centred by their own mean over
    all their nodes before the L2 normalisation (the item's seed frame included), which removes an appearance offset between the
    labelled radargram and this one.  memory_bias (needs memory; float, default 0.0): ``lp.propagate_all(memory_bias=)``, a bonus
    on the cosine of the long-term keys.  With None and 0.0 the call is bit for bit what it is without them."""
    crw_hip.check_memory_align(memory_align)
    memory_bias = crw_hip.check_memory_bias(memory_bias)
    if memory is None and (memory_align is not None or memory_bias != 0.0):
        raise ValueError("memory_align and memory_bias need memory: they say how a bank is brought to its item")
    if memory is not None:
        if not hasattr(lp, 'propagate_all'):
            raise ValueError("memory needs a label propagation with `propagate_all` (LabelPropVOS_CRW)")
        if novelty:
            raise ValueError("memory and novelty (suggest) are not combined: the novelty kernel scores against frame 0 and the window")
        if anchor_context != 'clamp':
            raise ValueError("memory and anchor_context='restart' are not combined: a restart drops every long-term frame but its origin")
        if getattr(lp, 'context', None) != 'sliding':
            from imported.labelprop import MEMORY_NEEDS_SLIDING
            raise ValueError(MEMORY_NEEDS_SLIDING)
        if memory.nodes != seq.shape[1] or tuple(memory.patches.shape[2:]) != tuple(seq.shape[2:]):
            raise ValueError(f"the bank's traces are {tuple(memory.patches.shape[1:])} (nodes, h, w), the item's frames "
                             f"{tuple(seq.shape[1:])}: a bank serves items of its own N and patch size")
    if confidence is not None and confidence not in crw_hip.CONF_KINDS:
        raise ValueError(f"confidence must be None or one of {', '.join(crw_hip.CONF_KINDS)} (got {confidence!r})")
    T, N, H, W = seq.shape
    if crw_hip.check_anchor_context(anchor_context) == 'restart' and anchors is None:
        raise ValueError("anchor_context='restart' needs anchors: a restart happens at a fully anchored frame")
    if anchors is not None:
        if not hasattr(lp, 'propagate_all'):
            raise ValueError("anchors need a label propagation with `propagate_all` (LabelPropVOS_CRW): the frame-by-frame protocol "
                             "of a foreign object has no place for them")
        if T > 1 and tuple(anchors.shape) != (T, N):
            raise ValueError(f"anchors must be [{T}, {N}] (got {tuple(anchors.shape)})")
    if novelty:
        if not hasattr(lp, 'propagate_all') or not hasattr(lp, 'novelty'):
            raise ValueError("novelty needs a label propagation with `propagate_all` and `novelty` (LabelPropVOS_CRW): a foreign "
                             "object's frame-by-frame protocol does not say which keys a frame scores against")
        crw_hip.novelty_top(N, novelty_top)
    mkw = {}
    if memory is None:
        feats, seed = _features_and_seed(seq, seg_ref, model, do_pos_embed, use_last)
    else:
        feats, seed, mem_feats = _features_and_seed(seq, seg_ref, model, do_pos_embed, use_last, memory, memory_align)
        mkw = dict(memory=(mem_feats, memory.labels.to(feats.device)))
        if memory_bias != 0.0:
            mkw.update(memory_bias=memory_bias)
        if T == 1 and seed is None:
            raise ValueError("a one-frame item without a seed has nothing to propagate from")
    if T == 1:  # a one-frame item (the correction step of test_all.py can ask for it): nothing to propagate, like the reference
        out = (seed[:, None].clone(), torch.zeros(N, 0), None)
        if confidence is not None:
            out += (torch.ones(N, 1, device=feats.device),)
        if novelty:
            out += ((torch.zeros(N, 1, device=feats.device), torch.zeros(1, device=feats.device)),)
        if soft:
            out += ((seed[:, None] == torch.arange(nclasses, device=feats.device)[None, :]).float(),)
        return out
    xent = crw_hip.xent_metric(feats)
    diffs = column_diffs_async(xent) if T > 2 else None  # on its way to the host before the label propagation is queued
    if anchors is not None:
        a = anchors.to(torch.int8)  # left where it is: from the host (`anchor_nodes`) the frames are found without a device read
        ckw = {} if anchor_context == 'clamp' else dict(anchor_context=anchor_context)
        pred, L = lp.propagate_all(feats, seed, nclasses, anchors=(torch.flip(a, (0,)) if use_last else a).contiguous(), **ckw, **mkw)
    elif hasattr(lp, 'propagate_all'):
        pred, L = lp.propagate_all(feats, seed, nclasses, **mkw)
    else:  # foreign label-propagation object: reference's frame-by-frame protocol
        pred = torch.zeros(N, T, device=feats.device)
        pred[:, 0] = seed
        mask = (seed[None, :] == torch.arange(nclasses, device=feats.device)[:, None]).float()[None, :, :, None]
        as_feat = lambda n: feats[n].t()[None, :, :, None]
        fl, ml = [as_feat(0)], [mask]
        for n in range(1, T):
            mask = lp.predict(feats=fl, masks=ml, curr_feat=as_feat(n))
            fl.append(as_feat(n))
            ml.append(mask)
            pred[:, n] = mask.argmax(1).squeeze()
        if confidence is not None or soft:  # the masks `predict` returned, [1,M,N,1] each, as the rows of L
            L = torch.cat(ml, 0)[..., 0].permute(0, 2, 1).reshape(T * N, nclasses).float().contiguous()
    # queued right behind the propagation, before the host turns to the change point
    conf = crw_hip.labelprop_confidence(L, T, N, nclasses, confidence) if confidence is not None else None
    nov = None
    if novelty:  # likewise queued behind the propagation, on the features it ran on
        nkw = {}
        if anchors is not None:
            nkw = dict(anchors=(torch.flip(a, (0,)) if use_last else a).contiguous(), anchor_context=anchor_context, nclasses=nclasses)
        nv, sc = lp.novelty(feats, top=novelty_top, **nkw)
        nov = (torch.cat([nv.new_zeros(N, 1), nv.t()], 1), torch.cat([sc.new_zeros(1), sc]))
    # the change point is host work (PELT on T-2 samples): it runs while the GPU propagates the labels queued above
    change_idx = change_point(xent, diffs)
    out = (pred, xent.cpu(), change_idx)
    if confidence is not None:
        out += (conf,)
    if novelty:
        out += (nov,)
    if soft:
        out += (L,)
    return out


def ndiag_matrix(size, n=1):
    """Row-normalised band matrix (n <= 2: identity, 3: tri-diagonal, ...)."""
    i = torch.arange(size)
    m = ((i[:, None] - i[None, :]).abs() <= max(n - 2, 0)).float()
    return m / m.sum(dim=1, keepdim=True)


@torch.no_grad()
def propagate_sweep(seq, seg_ref, model, sweep, nclasses, do_pos_embed, use_last, *, confidence=None, soft=False, anchors=None,
                    anchor_context='clamp', memory=None, memory_align=None):
    """`propagate` for every configuration of ``sweep`` (imported.labelprop.LabelPropSweep) at once: the encoder, the metric and
    the change point do not depend on (radius, temp, knn) and run ONCE, on the batch `propagate` gives the encoder
    ->  (labels [G,N,T] float, xent [N,T-1] (CPU), change_idx | None); labels[g] is `propagate`'s for ``sweep.configs[g]``.

    confidence / soft: the tuple grows as `propagate`'s does -- conf [G,N,T] float, then, last, the soft labels L [G, T*N, M]
    (frames in the pass's own order); conf[g] and L[g] are `propagate`'s for ``sweep.configs[g]``.  The confidence of all G
    configurations is ONE `crw_hip.labelprop_confidence` call on the stack read as G*T frames of one pass: the formula is per row,
    and every frame g*T is a one-hot seed, which reads 1.
    anchors: `propagate`'s -- [T, N] int8 in the ITEM's frame order, flipped here under ``use_last``, the same for all G
    configurations (``sweep`` under context 'sliding'); a one-frame item ignores them.  anchor_context: `propagate`'s.
    memory / memory_align: `propagate`'s -- the same `MemoryBank` in front of every configuration, encoded in the item's encoder
    call and centred as there; ``seg_ref`` may then be None.  The bias is not an argument: it is the sweep's own axis
    (``LabelPropSweep(biases=)``), and without a bank the sweep must not have one."""
    if confidence is not None and confidence not in crw_hip.CONF_KINDS:
        raise ValueError(f"confidence must be None or one of {', '.join(crw_hip.CONF_KINDS)} (got {confidence!r})")
    crw_hip.check_memory_align(memory_align)
    if memory is None and (memory_align is not None or list(getattr(sweep, 'biases', [0.0])) != [0.0]):
        raise ValueError("memory_align and memory_bias need memory: they say how a bank is brought to its item")
    if memory is not None:
        if anchor_context != 'clamp':
            raise ValueError("memory and anchor_context='restart' are not combined: a restart drops every long-term frame but its origin")
        if getattr(sweep, 'context', None) != 'sliding':
            from imported.labelprop import MEMORY_NEEDS_SLIDING
            raise ValueError(MEMORY_NEEDS_SLIDING)
        if memory.nodes != seq.shape[1] or tuple(memory.patches.shape[2:]) != tuple(seq.shape[2:]):
            raise ValueError(f"the bank's traces are {tuple(memory.patches.shape[1:])} (nodes, h, w), the item's frames "
                             f"{tuple(seq.shape[1:])}: a bank serves items of its own N and patch size")
    T, N, H, W = seq.shape
    if crw_hip.check_anchor_context(anchor_context) == 'restart' and anchors is None:
        raise ValueError("anchor_context='restart' needs anchors: a restart happens at a fully anchored frame")
    akw = {}
    if anchors is not None and T > 1:
        if tuple(anchors.shape) != (T, N):
            raise ValueError(f"anchors must be [{T}, {N}] (got {tuple(anchors.shape)})")
        a = anchors.to(torch.int8)
        akw = dict(anchors=(torch.flip(a, (0,)) if use_last else a).contiguous())
        if anchor_context != 'clamp':
            akw.update(anchor_context=anchor_context)
    if memory is None:
        feats, seed = _features_and_seed(seq, seg_ref, model, do_pos_embed, use_last)
    else:
        feats, seed, mem_feats = _features_and_seed(seq, seg_ref, model, do_pos_embed, use_last, memory, memory_align)
        akw.update(memory=(mem_feats, memory.labels.to(feats.device)))
        if T == 1 and seed is None:
            raise ValueError("a one-frame item without a seed has nothing to propagate from")
    G = len(sweep.configs)
    if T == 1:
        out = (seed[None, :, None].repeat(G, 1, 1), torch.zeros(N, 0), None)
        if confidence is not None:
            out += (torch.ones(G, N, 1, device=feats.device),)
        if soft:
            one_hot = (seed[:, None] == torch.arange(nclasses, device=feats.device)[None, :]).float()
            out += (one_hot[None].repeat(G, 1, 1),)
        return out
    xent = crw_hip.xent_metric(feats)
    diffs = column_diffs_async(xent) if T > 2 else None
    if confidence is None and not soft:
        pred = sweep.propagate_all(feats, seed, nclasses, **akw)
    else:
        pred, L = sweep.propagate_all(feats, seed, nclasses, soft=True, **akw)
    conf = None
    if confidence is not None:  # queued right behind the propagation, before the host turns to the change point
        conf = crw_hip.labelprop_confidence(L.reshape(G * T * N, nclasses), G * T, N, nclasses, confidence)  # [N, G*T]
        conf = conf.view(N, G, T).permute(1, 0, 2)
    change_idx = change_point(xent, diffs)  # host work while the GPU propagates
    out = (pred, xent.cpu(), change_idx)
    if confidence is not None:
        out += (conf,)
    if soft:
        out += (L,)
    return out
