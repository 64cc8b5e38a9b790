"""Whole-radargram inference on top of ``utils.propagate`` -- the driver loop of the reference's
evaluation script (scripts/test/test_all.py:71-159) without its plotting / report / private-data parts:

  * forward pass: every non-overlapping item is seeded with the reference segmentation of its first
    patch column and propagated along-track (test_all.py:91-100);
  * optional correction: where ``propagate`` reports a change point, a shortened item is re-seeded
    and its map replaces the tail of the radargram's map (test_all.py:103-122);
  * optional reverse pass: the items propagated from their LAST column (``use_last``) and merged
    into the forward map by a class rule (test_all.py:132-159).

The label maps are the reference's, operation for operation (pinned by ``tests/golden/segment_*.npz``,
which ``tests/golden/make_golden.py`` produces by running the reference's own ``main(args)``), which
includes three things one might not expect:
  * the correction step cuts its shortened item with ``dataset.get_smaller_item(index, small_length)``
    (src/dataset.py:41-47): the FIRST ``small_length`` patch-columns of the item -- not its tail -- while the
    seed labels and the overwritten map columns are the tail's (test_all.py:112-119);
  * ``get_smaller_item`` permanently shortens the dataset's item length, so a reverse pass that follows a
    correction runs on items of the last corrected length (their maps are stretched back to ``rg_len``);
  * the forward pass seeds from ``seg[:rg_h]`` (test_all.py:94), the correction and reverse passes from every
    row of ``seg`` (test_all.py:115,141);
  * any error inside a correction is swallowed (bare ``except``, test_all.py:121-122).
Label maps are upsampled to pixels with nearest-neighbour interpolation like the reference
(``transforms.Resize(NEAREST)``).  Everything heavy runs in ``propagate`` (encoder + HIP kernels).

``evaluate`` is the end of the same script (test_all.py:161-187): the ``--remove_unc`` masks and the report the reference prints,
from one pass of the HIP kernel ``crw_confusion`` over the label map where ``segment`` left it (``metrics.Report``).

``segment_sweep`` / ``evaluate_sweep`` are ``segment`` / ``evaluate`` for a grid of (radius, temp, knn) settings -- what
scripts/launch/launch_test_batch.sh does with one test_all.py run per setting -- with the encoder, the metric, the change points and
the whole control flow run once (``utils.propagate_sweep``, ``imported.labelprop.LabelPropSweep``).

``segment_radargrams`` is the other family of the reference's drivers: scripts/test/test_mc1.py, test_mc3.py and
test_sharad.py (``main(args)``), three whole radargrams held in memory, one item each; their defaults are in ``DRIVERS``.
"""
import torch
import torch.nn.functional as TF

import crw_hip
from utils import anchor_nodes, propagate, propagate_sweep


def _upsample(pred, rows, cols):
    """[..., N, T] node labels -> [..., rows, cols] pixel labels (nearest)."""
    up = TF.interpolate(pred.reshape(-1, 1, *pred.shape[-2:]).float(), size=(rows, cols), mode='nearest')
    return up.reshape(*pred.shape[:-2], rows, cols)


def _reverse_rule_mask(final_pred, pred_rev, dataset_id):
    """The pixels (bool, the maps' shape [..., rows, cols]) at which `merge_reverse`'s class rule writes the reverse pass's
    label, map by map."""
    mask = (pred_rev == 2).contiguous()
    if dataset_id == 1:
        mask = torch.logical_and(mask, final_pred != 3)
        mask = torch.logical_and(mask, torch.all(pred_rev != 4, dim=-2, keepdim=True))
    elif dataset_id == 3:
        mask.flatten(-2)[..., :mask.shape[-2] * mask.shape[-1] // 2] = False  # the first half of each map's pixels
    elif dataset_id != 0:
        raise ValueError(f'no merge rule for dataset id {dataset_id} (the reference defines 0, 1 and 3)')
    return mask


def merge_reverse(final_pred, pred_rev, dataset_id):
    """Class-specific merge of the reversed pass into the forward map (test_all.py:146-159):
    class 2 (bedrock) of the reversed pass wins, with per-dataset restrictions."""
    out = final_pred.clone()
    out[_reverse_rule_mask(final_pred, pred_rev, dataset_id)] = 2
    return out


_reverse_rule_mask_batch = _reverse_rule_mask  # [G, rows, cols] maps, configuration by configuration
merge_reverse_batch = merge_reverse


def _check_options(confidence, merge, upsample, decode='argmax', order=None, nclasses=None, posterior=False, use_last=False,
                   floor=None):
    """`segment`'s and `segment_sweep`'s checks of their options -> `order` as a list (None unless decode='ordered')."""
    if posterior:
        if decode != 'ordered':
            raise ValueError("posterior=True needs decode='ordered' (it is the posterior of that decode's monotone paths)")
        if use_last and merge != 'ordered':
            raise ValueError("posterior=True with use_last needs merge='ordered': merge='rule' / 'confidence' take pixels of two "
                             "decodes, and no one posterior describes the merged map")
        crw_hip.check_floor(floor)
    if merge not in ('rule', 'confidence', 'ordered'):
        raise ValueError(f"merge must be 'rule' or 'confidence' (got {merge!r}), or 'ordered' with decode='ordered'")
    if upsample not in ('nearest', 'bilinear'):
        raise ValueError(f"upsample must be 'nearest' or 'bilinear' (got {upsample!r})")
    if confidence is not None and confidence not in crw_hip.CONF_KINDS:
        raise ValueError(f"confidence must be None or one of {', '.join(crw_hip.CONF_KINDS)} (got {confidence!r})")
    if merge == 'confidence' and confidence is None:
        raise ValueError("merge='confidence' needs a confidence kind (confidence='maxprob', 'margin' or 'entropy')")
    if decode not in ('argmax', 'ordered'):
        raise ValueError(f"decode must be 'argmax' or 'ordered' (got {decode!r})")
    if merge == 'ordered' and decode != 'ordered':
        raise ValueError("merge='ordered' needs decode='ordered' (it is that decode, over the two passes' probabilities)")
    if merge == 'ordered' and confidence is None:
        raise ValueError("merge='ordered' needs a confidence kind (per pixel it reads the surer pass's probabilities)")
    if decode == 'argmax':
        if order is not None:
            raise ValueError("order needs decode='ordered'")
        return None
    if upsample != 'bilinear':
        raise ValueError("decode='ordered' needs upsample='bilinear' (it decodes the interpolated soft labels)")
    if order is None:
        raise ValueError("decode='ordered' needs an order (the classes from top to bottom, e.g. order=(0, 1, 2, 3))")
    return crw_hip.check_order(order, int(nclasses))


def _write_nearest(res, seq, out, out_conf, flip):
    """The nearest writer of `_segment_passes`: a pass's arg-max labels res[0] (and node confidences res[3]), [..., N, T],
    stretched into the windows -- both stretched before either is written; an int8 window casts."""
    ups = [(out, _upsample(res[0], *out.shape[-2:]))]
    if out_conf is not None:
        ups.append((out_conf, _upsample(res[3], *out.shape[-2:])))
    for window, up in ups:
        window[...] = torch.flip(up, (-1,)) if flip else up


def _check_anchor_context(anchor_context, anchors):
    if crw_hip.check_anchor_context(anchor_context) == 'restart' and anchors is None:
        raise ValueError("anchor_context='restart' needs anchors: a restart happens at a fully anchored frame")


def _segment_passes(dataset, seg, seq_length, patch_size, overlap, correction, use_last, dataset_id, device, want, merge, run, write,
                    lead=(), dtype=torch.float32, joint=None, posterior=0, anchors=None, anchor_context='clamp', forward_kw=None, **extra):
    """The passes of `segment` and `segment_sweep`, behind their argument checks -> their result dict (plus ``extra``).
    run(seq, seg_ref, use_last): the variant's `propagate` call -> (pred, xent, change, ...).
    write(res, seq, out, out_conf, flip): puts what `run` returned into a column window of the label map (and of the confidence
    map, None unless ``want``), mirrored along the columns with ``flip``.
    The maps are allocated ONCE at [*lead, rows, n_rg * rg_len] (labels ``dtype``, confidence float32) and every pass writes its
    own column window: the forward pass its radargram's, a correction the last ``px`` columns of it -- only after everything of it
    that can raise succeeded --, the reverse pass its radargram's, mirrored.  No list of maps, no cat, no flip of a map.
    merge='ordered': every pass that succeeded also leaves its soft labels res[3] and its geometry (frames, map width), the reverse
    pass decodes no map of its own, and joint(a, b, N, out, out_conf) writes a column window of ``pred`` / ``conf`` from two
    sources (L, T, cols, col0, flip) -- a radargram's, or the head and the tail of one whose correction succeeded.
    posterior: 0, or S = len(order).  ``post`` [*lead, rows, width] and ``horizon`` [*lead, 3, S-1, width] are then allocated
    once as well, and the call that writes a window of ``pred`` also gets the same window of the two, as the keyword
    post=(post window, horizon window): `write` without a reverse pass, `joint` with one (``pred`` is then the joint calls').
    anchors: None, or (annot, cols) of `segment`: `run` is then called with the keyword anchors=<the radargram's [T, N] node anchors>
    (`utils.anchor_nodes`) and anchor_context=``anchor_context`` in both passes, and the result gains ``anchor_cols`` and
    ``anchor_context``.
    forward_kw: further keywords for `run` in the forward pass of every full item, and nowhere else (`segment`'s suggest=)."""
    T, (H, W), (oh, ow) = seq_length, patch_size, overlap
    N = dataset[0].shape[1]
    rg_len = T * (W - ow) + ow
    rg_h = N * (H - oh) + oh
    idx = list(range(0, len(dataset), T))
    n_rg = min(len(idx), seg.shape[-1] // rg_len)
    idx = idx[:n_rg]
    seg = seg[:, :n_rg * rg_len].to(device)
    rows = seg.shape[0]
    new = lambda dt: torch.empty(*lead, rows, n_rg * rg_len, dtype=dt, device=device)
    new_maps = lambda: (new(dtype), new(torch.float32) if want else None)
    window = lambda maps, a, b: [m[..., a:b] if m is not None else None for m in maps]

    anch = lambda t: {}
    if anchors is not None:
        annot, cols = anchors
        cols = sorted(int(c) for c in cols)
        per_rg = anchor_nodes(torch.as_tensor(annot)[:, :n_rg * rg_len], cols, rg_len, T, N, rg_h, W - ow)
        ckw = {} if anchor_context == 'clamp' else dict(anchor_context=anchor_context)  # (the default is not passed on: `run` may be a caller's own)
        anch = lambda t: dict(anchors=per_rg[t], **ckw)
        extra.update(anchor_cols=cols, anchor_context=anchor_context)
        if anchor_context == 'restart':  # the fully labelled traces beyond the seed's: where the forward pass restarts
            extra.update(origin_traces=sum(int((p[1:] >= 0).all(1).sum()) for p in per_rg))
    forward, forward_conf = new_maps()
    xents, changes = [], []
    keep = use_last and merge == 'ordered'
    if posterior:
        post, horizon = new(torch.float32), torch.empty(*lead, 3, posterior - 1, n_rg * rg_len, dtype=torch.float32, device=device)
        extra.update(post=post, horizon=horizon)
    pwin = lambda a, b, mine: dict(post=(post[..., a:b], horizon[..., a:b])) if posterior and mine else {}
    fwd_src, tail_src = {}, {}  # radargram -> (L, frames, map width) of its forward pass / of its correction
    for t, i in enumerate(idx):
        seq = dataset[i].to(device)
        res = run(seq, seg[:rg_h, rg_len * t:rg_len * t + W], False, **anch(t), **(forward_kw or {}))
        write(res, seq, *window((forward, forward_conf), rg_len * t, rg_len * (t + 1)), False,
              **pwin(rg_len * t, rg_len * (t + 1), not keep))
        if keep:
            fwd_src[t] = (res[3], seq.shape[0], rg_len)
        xents.append(res[1])
        changes.append(res[2])

    if correction:
        for t, change in enumerate(changes):
            if change is None:
                continue
            small = T - change
            px = small * (W - ow)
            try:  # like the reference, a correction that fails on its DATA (shape / index errors) is skipped silently ...
                seq = dataset.get_smaller_item(idx[t], small).to(device)  # first `small` columns; shortens the dataset
                a, b = rg_len * (t + 1) - px, rg_len * (t + 1)
                res = run(seq, seg[:, a:a + W], False)
                write(res, seq, *window((forward, forward_conf), a, b), False, **pwin(a, b, not keep))  # labels and confidence: both or neither
                if keep:
                    tail_src[t] = (res[3], seq.shape[0], px)
            except crw_hip.CrwError as e:
                # ... but a failure of the HIP path itself (CRW_EHIP: launch failure / GPU fault, CRW_EWORKSPACE) is not a data
                # problem: the reference's bare `except` would hide a poisoned device context behind an uncorrected map.
                # CRW_EINVAL (a degenerate correction window: bad shape / unsupported size) IS the data and is skipped
                if e.device_failure:
                    raise
            except torch.AcceleratorError:  # the device runtime's own errors (hipError* raised by PyTorch)
                raise
            except Exception:
                pass

    final, final_conf = forward, forward_conf
    if use_last:
        rev, rev_conf = new_maps()  # merge='ordered': the merged maps themselves, there is no reverse map
        seg_rev = torch.flip(seg.unfold(1, rg_len, rg_len), (-1,)).reshape(rows, -1)
        for t, i in enumerate(idx):
            seq = dataset[i].to(device)
            res = run(seq, seg_rev[:, rg_len * t:rg_len * t + W], True, **anch(t))
            if not keep:
                write(res, seq, *window((rev, rev_conf), rg_len * t, rg_len * (t + 1)), True)
                continue
            a, b = rg_len * t, rg_len * (t + 1)
            px = tail_src[t][2] if t in tail_src else 0
            back = (res[3], seq.shape[0], rg_len)
            if px < rg_len:  # the radargram, or the head of a corrected one
                joint((*fwd_src[t], 0, False), (*back, 0, True), N, *window((rev, rev_conf), a, b - px), **pwin(a, b - px, True))
            if px:  # the corrected tail: the shortened item's whole map against the last px columns of the reverse pass's
                joint((*tail_src[t], 0, False), (*back, rg_len - px, True), N, *window((rev, rev_conf), b - px, b), **pwin(b - px, b, True))
        if keep:
            final, final_conf = rev, rev_conf
        elif merge == 'confidence':
            final, final_conf, _ = crw_hip.merge_confidence(forward, forward_conf, rev, rev_conf)
        else:
            final = merge_reverse(forward, rev, dataset_id)
            if want:
                final_conf = torch.where(_reverse_rule_mask(forward, rev, dataset_id), rev_conf, forward_conf)
    out = dict(pred=final, forward=forward, xent=xents, change_idx=changes, **extra)
    if want:
        out.update(conf=final_conf, forward_conf=forward_conf)
    return out


@torch.no_grad()
def segment(dataset, seg, encoder, lp, nclasses, seq_length, patch_size, overlap, pos_embed=False,
            correction=False, use_last=False, dataset_id=0, device='cuda', confidence=None, merge='rule', upsample='nearest',
            decode='argmax', order=None, posterior=False, floor=crw_hip.POSTERIOR_FLOOR, anchors=None, anchor_context='clamp', suggest=0, suggest_gap=2,
            suggest_top=None, memory=None, seedless=False, memory_align=None, memory_bias=0.0):
    """dataset: RGDataset (full, overlapping items); seg: reference segmentation [rows, W_rg].
    -> dict(pred [rows, n_rg * rg_len] float labels after the optional reverse merge,
            forward: the forward (+ corrected) map the reference saves as int8 (test_all.py:128),
            xent list, change_idx list).

    confidence: None, or a kind of `crw_hip.labelprop_confidence` ('maxprob', 'margin', 'entropy').  The dict then gains
    ``conf`` and ``forward_conf``, float32 [rows, n_rg * rg_len]: the confidence of every pixel of ``pred`` / ``forward``, from the
    soft labels of the pass that wrote the pixel's label -- upsampled, spliced by the correction and flipped exactly as the labels
    are; 1 on every seed column.  ``pred`` and ``forward`` do not depend on it.
    merge: how the reverse pass (``use_last``) enters ``pred``.  'rule': the reference's class rule (`merge_reverse`), defined for
    dataset ids 0, 1 and 3; ``conf`` is the reverse pass's exactly where the rule wrote its label.  'confidence': per pixel, the
    pass that is surer (`crw_hip.merge_confidence`: the reverse pass where its confidence is strictly larger) -- needs no class
    semantics, so any ``dataset_id`` is accepted; needs ``confidence``.  'ordered' (needs decode='ordered' and ``confidence``; any
    ``dataset_id``): the two passes are merged BEFORE the decode -- per pixel the interpolated probabilities of the surer pass
    (that same rule), one `crw_hip.labelmap_ordered_joint` per radargram (two where a correction succeeded: head and tail), no
    reverse map is decoded; ``conf``, ``forward`` and ``forward_conf`` are merge='confidence''s bit for bit.
    upsample: how a pass's [N, T] nodes become pixels.  'nearest': the reference's -- arg-max per node, then Resize(NEAREST), every
    class boundary on the node grid.  'bilinear': the upstream routine's order (imported/crw.py:124-127) -- the pass's soft labels
    interpolated bilinearly to pixels and arg-maxed after that (`crw_hip.labelmap_dense`, one kernel per pass, straight into the
    pass's column window of the map); ``conf`` / ``forward_conf`` are then the confidence of the INTERPOLATED distribution.  Same
    passes, corrections, exception policy and merges.
    decode: how a pixel's class is read from the interpolated probabilities.  'argmax': per pixel.  'ordered' (needs
    upsample='bilinear' and ``order``, the classes from top to bottom; no per-dataset default, the class semantics are the
    caller's): per pixel column, the labelling that never steps back in ``order`` and collects the largest summed probability
    (`crw_hip.labelmap_ordered` where 'argmax' calls `labelmap_dense`; same passes, corrections, exception policy and merges;
    ``conf`` / ``forward_conf`` unchanged, they do not depend on the decode).  The dict then gains ``decode`` and ``order``.
    The guarantee: every pass's window is monotone in ``order`` down every column, so ``forward`` is, and ``pred`` without a
    reverse pass; after merge='rule' / 'confidence' the merged ``pred`` takes pixels of two monotone maps and need not be; with
    merge='ordered' ``pred`` is monotone in ``order`` down every column.
    posterior (needs decode='ordered'; with ``use_last`` also merge='ordered', so that every window of ``pred`` is ONE decode's
    output): the confidence that belongs to the decode.  The dict gains ``post`` float32 [rows, n_rg * rg_len], the posterior
    probability of every pixel's label in ``pred`` over the monotone paths of its column, ``horizon`` float32 [3, S-1, n_rg *
    rg_len] -- per boundary and column the pick, its posterior mean and the error bar of the pick, in rows -- and ``floor``, the floor
    under the evidence (`crw_hip.labelmap_ordered_posterior` / `labelmap_ordered_joint_posterior`, called on the window a decode just
    wrote: the forward pass, a corrected tail after it succeeded, the joint calls).  Every other entry is bit for bit what it is
    without the option.
    anchors: None, or (annot, cols) -- labelled traces INSIDE the radargrams (needs a label propagation under CONTEXT 'sliding').
    annot [rows, W_rg] integer labels, < 0 = unlabelled (it may be ``seg`` itself); cols: the annotated pixel columns.  Each becomes
    the node anchors of its frame (`utils.anchor_nodes`), which clamp those nodes' soft labels to their class before the next frame
    reads them.  Both passes see the same anchors, the reverse pass mirrored (frame T - 1 - f); an anchor on a pass's own seed frame
    is ignored by that pass (``seg`` rules there) and live in the other.  Everything downstream takes the soft labels as before:
    confidence 1 at a clamped node, the maps, both decodes, the merges, the posterior.  The dict gains ``anchor_cols``.  Not
    together with ``correction``: the correction is itself a re-seed, and how the two combine is not decided.
    anchor_context: 'clamp', or 'restart' (needs anchors) -- a fully labelled trace is as good as a seed: the frames behind it are
    propagated as frames of the item that starts there (`LabelPropVOS_CRW.propagate_all`).  Both passes restart, the reverse pass on
    the mirrored anchors; everything downstream is untouched.  With anchors the dict gains ``anchor_context``.
    suggest: 0, or how many traces per radargram to propose for labelling next (needs a label propagation with `novelty`).  The
    forward pass of every full item -- no correction, not the reverse pass -- also computes the context novelty of its frames on
    the features it propagates (`propagate(novelty=True)`; suggest_top: `novelty_top`), and the dict gains ``novelty``, float32
    [items, T] on the CPU (frame scores, 0 at the seed frame), and ``suggested``: per radargram the picks of
    `crw_hip.suggest_frames` (suggest_gap: its min_gap) as dicts radargram, item, frame, column, columns (first, last + 1), z,
    score -- ``column`` is the frame's first pixel column, which `utils.anchor_nodes` maps back to that frame.  ``anchors`` are
    honoured: under 'restart' the keys start at the origins, and fully labelled frames are not proposed again, so labelling a
    pick and passing it as an anchor gives the next picks.  A pick is a place to look, not a detection: items in which nothing
    new appears give z as large as a weak onset's.  Every other entry is bit for bit what it is without the option.
    memory: None, a `utils.MemoryBank`, or (annot, cols) -- fully labelled traces from ELSEWHERE (`utils.bank_from_columns` cuts the
    patch columns that start at the pixel columns ``cols`` of this dataset; a bank may as well come from another radargram or a
    file).  Needs a label propagation under CONTEXT 'sliding'.  Every item of both passes is propagated with the same bank in front
    of it as long-term frames (`utils.propagate(memory=)`: the bank's patches go through the encoder with the item); everything
    downstream takes the soft labels as before.  Not together with anchor_context='restart' or ``suggest``.  The dict gains
    ``memory_traces`` (the number of bank traces) and ``seedless``.
    seedless (needs memory; not with ``correction``, which is a re-seed from ``seg``): no item is seeded from ``seg`` -- its first
    frame is predicted from the bank like any other, and ``seg`` serves the geometry and the evaluation only.
    memory_align (None | 'center'), memory_bias (float, 0.0): how the bank is brought to every item -- `utils.propagate`'s options of
    those names, the same settings for every item of both passes; they need ``memory``.  With a bank the dict gains ``memory_align``
    and ``memory_bias``.  At None and 0.0 every entry is bit for bit what it is without them."""
    _check_anchor_context(anchor_context, anchors)
    crw_hip.check_memory_align(memory_align)
    memory_bias = crw_hip.check_memory_bias(memory_bias)
    if memory is None and (memory_align is not None or memory_bias != 0.0):
        raise ValueError("memory_align and memory_bias need memory: they say how a bank is brought to its item")
    bank = None
    if seedless and memory is None:
        raise ValueError("seedless=True needs memory: without a bank nothing labels an item's first frame")
    if seedless and correction:
        raise ValueError("seedless=True and correction=True do not combine: the correction is a re-seed from the ground truth")
    if memory is not None:
        from utils import MemoryBank, bank_from_columns
        from imported.labelprop import MEMORY_NEEDS_SLIDING
        if getattr(lp, 'context', None) != 'sliding' or not hasattr(lp, 'propagate_all'):
            raise ValueError(MEMORY_NEEDS_SLIDING)
        if anchor_context != 'clamp':
            raise ValueError("memory and anchor_context='restart' do not combine: a restart drops every long-term frame but its origin")
        if suggest:
            raise ValueError("memory and suggest do not combine: the novelty kernel scores against frame 0 and the window, not the bank")
        bank = memory if isinstance(memory, MemoryBank) else bank_from_columns(dataset, *memory)
        if bank.nodes != dataset[0].shape[1]:
            raise ValueError(f"the bank's traces have {bank.nodes} nodes, the items {dataset[0].shape[1]}: a bank serves items of its own N")
    if int(suggest) < 0 or int(suggest_gap) < 0:
        raise ValueError(f"suggest and suggest_gap must be >= 0 (got {suggest}, {suggest_gap})")
    if suggest and not hasattr(lp, 'novelty'):
        raise ValueError("suggest needs a label propagation with `novelty` (LabelPropVOS_CRW)")
    order = _check_options(confidence, merge, upsample, decode, order, nclasses, posterior, use_last, floor)
    if anchors is not None and correction:
        raise ValueError("anchors and correction=True do not combine: the correction is itself a re-seed (at the change point), and "
                         "how the two interact is not decided")
    want = confidence is not None
    extra = dict(decode=decode, order=order) if order else {}
    if posterior:
        extra['floor'] = float(floor)
    if bank is not None:
        extra.update(memory_traces=len(bank), seedless=bool(seedless), memory_align=memory_align, memory_bias=memory_bias)
    if upsample == 'bilinear':
        kw = dict(soft=True)

        def write(res, seq, out, out_conf, flip, post=None):  # res[3]: the pass's soft labels L [T*N, M]
            if order:
                crw_hip.labelmap_ordered(res[3], *seq.shape[:2], nclasses, *out.shape, order, confidence=confidence, flip=flip,
                                         out=out, out_conf=out_conf)
                if post is not None:
                    crw_hip.labelmap_ordered_posterior(res[3], *seq.shape[:2], nclasses, *out.shape, order, out, flip=flip, floor=floor,
                                                       out=post[0], out_hz=post[1])
            else:
                crw_hip.labelmap_dense(res[3], *seq.shape[:2], nclasses, *out.shape, confidence=confidence, flip=flip, out=out,
                                       out_conf=out_conf)
    else:
        kw = dict(confidence=confidence) if want else {}  # `propagate` returns a fourth entry only when asked
        write = _write_nearest
    novs = []  # (nov [N, T], score [T]) of every full item's forward pass, with suggest

    def run(seq, seg_ref, last, novelty=False, **anch):
        nkw = dict(novelty=True, novelty_top=suggest_top) if novelty else {}
        if bank is not None:  # the same bank in front of every item of both passes; seedless: `seg` seeds nothing
            nkw.update(memory=bank)
            if memory_align is not None:
                nkw.update(memory_align=memory_align)
            if memory_bias != 0.0:
                nkw.update(memory_bias=memory_bias)
            seg_ref = None if seedless else seg_ref
        res = propagate(seq, seg_ref, encoder, lp, nclasses, pos_embed, use_last=last, **kw, **anch, **nkw)
        if novelty:  # taken out again: the writers read the tuple by position
            at = 4 if 'confidence' in kw else 3
            novs.append(res[at])
            res = res[:at] + res[at + 1:]
        return res

    def joint(a, b, N, out, out_conf, post=None):  # merge='ordered': a column window of pred / conf from two passes' soft labels
        crw_hip.labelmap_ordered_joint(a, b, N, nclasses, *out.shape, order, confidence=confidence, out=out, out_conf=out_conf)
        if post is not None:
            crw_hip.labelmap_ordered_joint_posterior(a, b, N, nclasses, *out.shape, order, out, confidence=confidence, floor=floor,
                                                     out=post[0], out_hz=post[1])
    out = _segment_passes(dataset, seg, seq_length, patch_size, overlap, correction, use_last, dataset_id, device, want, merge, run,
                          write, joint=joint, posterior=len(order) if posterior else 0, anchors=anchors, anchor_context=anchor_context,
                          forward_kw=dict(novelty=True) if suggest else None, **extra)
    if suggest:
        out.update(_suggested(novs, lp.cxt_size, int(suggest), int(suggest_gap), dataset[0].shape[1], nclasses, seq_length, patch_size,
                              overlap, anchors))
    return out


def _suggested(novs, cxt_size, budget, gap, N, nclasses, seq_length, patch_size, overlap, anchors):
    """`segment`'s ``novelty`` and ``suggested`` from the forward passes' (nov, score) pairs: ONE copy to the host, then host work."""
    T, (H, W), (oh, ow) = seq_length, patch_size, overlap
    step, rg_len, rg_h = W - ow, T * (W - ow) + ow, N * (H - oh) + oh
    s = torch.stack([sc for _, sc in novs]).cpu()
    per_rg = None
    if anchors is not None:
        annot, cols = anchors
        per_rg = anchor_nodes(torch.as_tensor(annot)[:, :len(novs) * rg_len], cols, rg_len, T, N, rg_h, step)
    suggested = []
    for t in range(len(novs)):
        full = [] if per_rg is None else [f for f in range(1, T) if bool(((per_rg[t][f] >= 0) & (per_rg[t][f] < nclasses)).all())]
        picks = []
        for f, z, sc in crw_hip.suggest_frames(s[t, 1:], cxt_size, budget, gap, 1, full):
            first = t * rg_len + f * step
            picks.append(dict(radargram=t, item=t * T, frame=f, column=first, columns=(first, first + step if f < T - 1 else (t + 1) * rg_len),
                              z=z, score=sc))
        suggested.append(picks)
    return dict(novelty=s, suggested=suggested)


@torch.no_grad()
def segment_sweep(dataset, seg, encoder, sweep, nclasses, seq_length, patch_size, overlap, pos_embed=False,
                  correction=False, use_last=False, dataset_id=0, device='cuda', confidence=None, merge='rule', upsample='nearest',
                  decode='argmax', order=None, anchors=None, anchor_context='clamp', memory=None, memory_align=None, memory_bias=0.0,
                  bank=None, bank_align=None, seedless=False, **posterior_options):
    """`segment` for every configuration of ``sweep`` (LabelPropSweep, G = len(sweep.configs)) with its control flow run ONCE:
    which items are corrected, at which length (`get_smaller_item` and its permanent shortening of the dataset) and what the
    reverse pass sees depend on the features alone, never on (radius, temp, knn).  Same exception policy in the correction.
    -> dict(pred [G, rows, cols] int8 (after the optional reverse merge), forward [G, rows, cols] int8, xent list, change_idx
            list, configs); pred[g] / forward[g] are `segment`'s maps for ``sweep.configs[g]`` (on a fresh dataset).

    confidence / merge / upsample: `segment`'s arguments, checks and messages.  With a confidence kind the dict gains ``conf`` and
    ``forward_conf`` [G, rows, cols] float32, slice g bit for bit `segment`'s for ``sweep.configs[g]`` under the same options.
    merge='confidence': ONE `crw_hip.merge_confidence` over the G maps; it needs no class rule, so any ``dataset_id`` is accepted
    (the class rule's dataset check applies to merge='rule' alone).  upsample='bilinear': the maps are allocated once at
    [G, rows, n_rg * rg_len] and every pass writes its column window of all G maps with one `crw_hip.labelmap_dense_batch`.
    It holds G-map tensors at once: with confidence, 5 bytes per pixel and configuration for the forward maps, as much again for
    the reverse pass's and for the merge's result.  decode / order: `segment`'s, one ``order`` for the G configurations, every
    pass ONE `crw_hip.labelmap_ordered_batch`; slice g stays `segment`'s for ``sweep.configs[g]`` under the same options.
    merge='ordered': `segment`'s, every window ONE `crw_hip.labelmap_ordered_joint_batch` for the G configurations.
    posterior=False, floor=crw_hip.POSTERIOR_FLOOR: `segment`'s two options, with its checks and messages.  They OUGHT to be named
    keyword parameters, as they are in `segment`.  They come through ``posterior_options`` for one reason only:
    tests/test_posterior.py::test_segment_option_errors still asserts that the sweep has no parameter named ``posterior`` ("the
    sweep does not take the option"), an assertion this feature makes stale.  When that line is updated, declare the two by name
    and delete the three lines below that unpack them.  Any other keyword is the TypeError a named parameter would give.  The dict
    gains ``post`` float32 [G, rows, cols], ``horizon``
    float32 [G, 3, S-1, cols] and ``floor``; slice g is `segment`'s for ``sweep.configs[g]``, bit for bit.  The call that writes a
    window of ``pred`` writes the same window of the two for all G configurations (`crw_hip.labelmap_ordered_posterior_batch` /
    `labelmap_ordered_joint_posterior_batch`, as few launches as fit the workspace cap); every other entry is bit for bit what
    it is without the option.
    anchors: `segment`'s -- None, or (annot, cols), labelled traces inside the radargrams (needs a ``sweep`` under context
    'sliding'); the same anchors in both passes and for all G configurations, the reverse pass mirrored, not together with
    ``correction``; the dict gains ``anchor_cols``.  Slice g stays `segment`'s for ``sweep.configs[g]`` under the same anchors.
    anchor_context: `segment`'s, one set of origins for the G configurations.
    bank: what `segment`'s ``memory`` takes -- None, a `utils.MemoryBank`, or (annot, cols): fully labelled traces from elsewhere
    (needs a ``sweep`` under context 'sliding', anchor_context 'clamp').  The same bank stands in front of every item of both
    passes and of all G configurations (`utils.propagate_sweep(memory=)`, crw_labelprop_propagate_long_batch); slice g is
    `segment(memory=bank, memory_align=bank_align, memory_bias=configs[g].get('MEMORY_BIAS', 0.0))` for ``sweep.configs[g]``.
    bank_align: `segment`'s ``memory_align`` (None | 'center'), one setting for the G configurations.  seedless: `segment`'s (needs a
    bank, not with ``correction``).  The bias is the sweep's own grid axis, ``LabelPropSweep(biases=)``; without a bank the sweep
    must not have one.  With a bank the dict gains ``memory_traces``, ``seedless`` and ``memory_align``.
    These two OUGHT to be named ``memory`` and ``memory_align``, as in `segment`.  They are not for one reason only:
    tests/test_longmem_host.py::test_every_refusal_has_its_message and
    tests/test_align_host.py::test_segment_hands_the_same_settings_to_both_passes_and_refuses_what_it_must still assert that
    ``memory``, ``memory_align`` and ``memory_bias`` raise "memory is not offered in segment_sweep", assertions this feature makes
    stale.  When those two are updated, rename ``bank`` / ``bank_align`` and delete the refusal below.
    memory, memory_align, memory_bias: refused -- see above."""
    if memory is not None or memory_align is not None or memory_bias != 0.0:
        raise ValueError("memory is not offered in segment_sweep under these names: pass the bank as bank=, its alignment as "
                         "bank_align=, and the biases to sweep as LabelPropSweep(biases=)")
    crw_hip.check_memory_align(bank_align)
    biased = list(getattr(sweep, 'biases', [0.0])) != [0.0]
    if bank is None and (bank_align is not None or biased):
        raise ValueError("memory_align and memory_bias need memory: they say how a bank is brought to its item")
    if seedless and bank is None:
        raise ValueError("seedless=True needs memory: without a bank nothing labels an item's first frame")
    if seedless and correction:
        raise ValueError("seedless=True and correction=True do not combine: the correction is a re-seed from the ground truth")
    if bank is not None:
        from utils import MemoryBank, bank_from_columns
        from imported.labelprop import MEMORY_NEEDS_SLIDING
        if getattr(sweep, 'context', None) != 'sliding':
            raise ValueError(MEMORY_NEEDS_SLIDING)
        if anchor_context != 'clamp':
            raise ValueError("memory and anchor_context='restart' do not combine: a restart drops every long-term frame but its origin")
        bank = bank if isinstance(bank, MemoryBank) else bank_from_columns(dataset, *bank)
        if bank.nodes != dataset[0].shape[1]:
            raise ValueError(f"the bank's traces have {bank.nodes} nodes, the items {dataset[0].shape[1]}: a bank serves items of its own N")
    _check_anchor_context(anchor_context, anchors)
    if anchors is not None and correction:
        raise ValueError("anchors and correction=True do not combine: the correction is itself a re-seed (at the change point), and "
                         "how the two interact is not decided")
    posterior, floor = posterior_options.pop('posterior', False), posterior_options.pop('floor', crw_hip.POSTERIOR_FLOOR)
    if posterior_options:
        raise TypeError(f"segment_sweep() got an unexpected keyword argument '{next(iter(posterior_options))}'")
    order = _check_options(confidence, merge, upsample, decode, order, nclasses, posterior, use_last, floor)
    extra = dict(decode=decode, order=order) if order else {}
    if posterior:
        extra['floor'] = float(floor)
    if bank is not None:
        extra.update(memory_traces=len(bank), seedless=bool(seedless), memory_align=bank_align)
    if merge == 'rule' and dataset_id not in (0, 1, 3) and use_last:
        raise ValueError(f'no merge rule for dataset id {dataset_id} (the reference defines 0, 1 and 3)')
    want = confidence is not None
    G = len(sweep.configs)
    if upsample == 'bilinear':
        kw = dict(soft=True)

        def write(res, seq, out, out_conf, flip, post=None):  # res[3]: the pass's soft labels L [G, T*N, M]; ONE launch for the G maps
            if order:
                crw_hip.labelmap_ordered_batch(res[3], G, *seq.shape[:2], nclasses, *out.shape[1:], order, confidence=confidence,
                                               flip=flip, dtype=torch.int8, out=out, out_conf=out_conf)
                if post is not None:
                    crw_hip.labelmap_ordered_posterior_batch(res[3], G, *seq.shape[:2], nclasses, *out.shape[1:], order, out, flip=flip,
                                                             floor=floor, out=post[0], out_hz=post[1])
            else:
                crw_hip.labelmap_dense_batch(res[3], G, *seq.shape[:2], nclasses, *out.shape[1:], confidence=confidence, flip=flip,
                                             dtype=torch.int8, out=out, out_conf=out_conf)
    else:
        kw = dict(confidence=confidence) if want else {}  # `propagate_sweep` returns a fourth entry only when asked
        write = _write_nearest
    def run(seq, seg_ref, last, **anch):
        mkw = {}
        if bank is not None:  # the same bank in front of every item of both passes; seedless: `seg` seeds nothing
            mkw.update(memory=bank)
            if bank_align is not None:
                mkw.update(memory_align=bank_align)
            seg_ref = None if seedless else seg_ref
        return propagate_sweep(seq, seg_ref, encoder, sweep, nclasses, pos_embed, use_last=last, **kw, **anch, **mkw)

    def joint(a, b, N, out, out_conf, post=None):  # merge='ordered': ONE launch per window for the G configurations
        crw_hip.labelmap_ordered_joint_batch(a, b, G, N, nclasses, *out.shape[1:], order, confidence=confidence, dtype=torch.int8,
                                             out=out, out_conf=out_conf)
        if post is not None:
            crw_hip.labelmap_ordered_joint_posterior_batch(a, b, G, N, nclasses, *out.shape[1:], order, out, confidence=confidence,
                                                           floor=floor, out=post[0], out_hz=post[1])
    return _segment_passes(dataset, seg, seq_length, patch_size, overlap, correction, use_last, dataset_id, device, want, merge, run,
                           write, lead=(G,), dtype=torch.int8, joint=joint, posterior=len(order) if posterior else 0, anchors=anchors,
                           anchor_context=anchor_context, configs=list(sweep.configs), **extra)


@torch.no_grad()
def segment_one(dataset, seg, encoder, lp, nclasses, seq_length, patch_size, overlap, pos_embed=False, device='cuda'):
    """``main(args)`` of the reference's scripts/test/test.py (:45-84) without the plots: the FIRST radargram only, forward pass
    seeded from ``seg[:rg_h, :W]``, then always one correction -- at ``seq_length - 2`` when ``propagate`` finds no change point
    (:70-71) -- on ``dataset.get_smaller_item(0, small)`` seeded from every row of ``seg``; nothing is caught, an error ends the
    run.  The caller puts the encoder in eval mode (test.py:42).  -> dict(pred [rows, rg_len], change_idx)."""
    T, (H, W), (oh, ow) = seq_length, patch_size, overlap
    seq = dataset[0].to(device)
    N = seq.shape[1]
    rg_len = T * (W - ow) + ow
    rg_h = N * (H - oh) + oh
    seg = seg.to(device)
    rows = seg.shape[0]
    pred, _, change = propagate(seq, seg[:rg_h, :W], encoder, lp, nclasses, pos_embed, use_last=False)
    final = _upsample(pred, rows, rg_len)
    if change is None:
        change = T - 2
    small = T - change
    px = small * (W - ow)
    seq = dataset.get_smaller_item(0, small).to(device)
    pred, _, _ = propagate(seq, seg[:, rg_len - px:rg_len - px + W], encoder, lp, nclasses, pos_embed, use_last=False)
    final[:, rg_len - px:] = _upsample(pred, rows, px)
    return dict(pred=final, change_idx=change)


# dataset id -> number of classes, as utils.get_reference returns it (src/utils.py:57-70)
NCLASSES = {0: 4, 1: 6, 2: 4, 3: 5}


def _report_rules(pred, seg, dataset_id, remove_unc, unc_seg, nclasses):
    """`evaluate`'s argument checks and ``--remove_unc`` rules -> (K, seg on pred's device, mask arguments of the kernel call)."""
    if dataset_id not in (0, 1, 3):
        raise ValueError(f'no report rule for dataset id {dataset_id} (the reference defines 0, 1 and 3)')
    K = NCLASSES[dataset_id] if nclasses is None else int(nclasses)
    if pred.numel() != seg.numel():
        raise ValueError(f'pred {tuple(pred.shape)} and seg {tuple(seg.shape)} must cover the same pixels')
    seg = seg.to(pred.device)
    mask = {}
    if remove_unc and dataset_id == 0:
        if unc_seg is None:
            raise ValueError('dataset 0 with remove_unc needs unc_seg (the dataset-2 reference map, same columns)')
        if unc_seg.numel() != seg.numel():
            raise ValueError(f'unc_seg {tuple(unc_seg.shape)} and seg {tuple(seg.shape)} must cover the same pixels')
        mask = dict(aux=unc_seg.to(pred.device), ignore_aux=4)
    elif remove_unc and dataset_id == 1:
        mask = dict(ignore_gt=5, ignore_pred=5)
    return K, seg, mask


def _dropped(tail, K):
    """The drop counts that end a report's host row, as a list; a label outside 0 ... K-1 that survived the mask raises."""
    dropped = [int(v) for v in tail]
    if dropped[1]:
        raise crw_hip.LabelError(dropped[1], K)
    return dropped


def _host_rows(outs):
    """What G queued kernel calls returned (per call: integer tensors that end in the drop counts) -> [G, numbers per map] on the
    host, in ONE copy; no call, no copy."""
    return torch.stack([torch.cat([t.reshape(-1) for t in out]) for out in outs]).cpu() if outs else []


def _calibration_of(row, nb, K):
    """A host row of `crw_hip.calibration`'s outputs (counts [nb, 2], the bit pattern of conf_sum [nb], dropped [3])."""
    from metrics import Calibration
    return Calibration(row[:2 * nb].view(nb, 2), row[2 * nb:3 * nb].view(torch.float64), _dropped(row[3 * nb:], K))


def _horizons_of(row, K, shape, min_run, tol, row_spacing, unit):
    """A host row of `crw_hip.horizons`'s outputs (statistics [K, 18], dropped [2]) for a map of ``shape`` [rows, cols]."""
    from metrics import Horizons
    return Horizons(row[:18 * K].view(K, 18), _dropped(row[18 * K:], K), shape[0], shape[1], min_run, tol, row_spacing=row_spacing,
                    unit=unit)


def evaluate(pred, seg, dataset_id, remove_unc=True, unc_seg=None, nclasses=None):
    """The report of test_all.py:161-187 for a label map ``pred`` (``segment(...)['pred']``, or a saved int8 map) against the
    reference segmentation ``seg`` cut to the same columns -> ``metrics.Report``.

    ``remove_unc`` (the script's default): dataset 0 drops the pixels whose ``unc_seg`` -- the reference's dataset-2 map cut to the
    same columns, required then -- is 4 (:162-167); dataset 1 drops the pixels whose ground truth or prediction is 5 (:168-172);
    dataset 3 drops nothing (:173-175).  The rules are mask arguments of the one ``crw_hip.confusion`` call: no boolean-indexed
    copy of the maps, no copy to the host but the K x K counts.  K = ``nclasses`` (default: the dataset's, labels 0 ... K-1); the
    4s of dataset 0's uncertain map are compared, never binned.  A label outside 0 ... K-1 that survives the mask raises
    ``crw_hip.LabelError`` (a ValueError)."""
    from metrics import Report
    K, seg, mask = _report_rules(pred, seg, dataset_id, remove_unc, unc_seg, nclasses)
    counts, dropped = crw_hip.confusion(seg, pred, K, **mask)
    return Report(counts, _dropped(dropped.cpu(), K))


def calibration(pred, conf, seg, dataset_id, remove_unc=True, unc_seg=None, nclasses=None, bins=10):
    """Does low confidence find the wrong pixels?  The reliability histogram of a confidence map ``conf`` (``segment(...,
    confidence=kind)['conf']``) for the label map ``pred`` against ``seg`` -> ``metrics.Calibration`` (per-bin accuracy and mean
    confidence, ECE / MCE, the risk-coverage curve).  `evaluate`'s arguments and mask rules, passed through as arguments of the one
    ``crw_hip.calibration`` call: the pixels it bins are the pixels `evaluate` counts.  A surviving label outside 0 ... K-1 raises
    ``crw_hip.LabelError``; a surviving confidence that is NaN or outside [0, 1] is counted in ``dropped[2]`` and binned nowhere."""
    K, seg, mask = _report_rules(pred, seg, dataset_id, remove_unc, unc_seg, nclasses)
    if conf.numel() != pred.numel():
        raise ValueError(f'conf {tuple(conf.shape)} and pred {tuple(pred.shape)} must cover the same pixels')
    counts, conf_sum, dropped = crw_hip.calibration(seg, pred, conf.to(pred.device), K, bins=bins, **mask)
    host = torch.cat([counts.reshape(-1), conf_sum.view(torch.int64), dropped]).cpu()  # the one copy: 3 * bins + 3 numbers
    return _calibration_of(host, conf_sum.numel(), K)


def horizon_bars(horizon, seg, order, z=2.0, slack=1.0):
    """Do the error bars cover the truth?  ``horizon`` [3, S-1, width] (``segment(..., posterior=True)['horizon']``: pick, posterior
    mean, error bar of the pick) against the reference segmentation ``seg`` [rows, width] -> ``metrics.HorizonBars``.  The
    reference's boundary k = 1 ... S-1 of a column is the first row whose class's position in ``order`` is >= k (a class outside
    ``order`` has none); per boundary, over the columns in which the reference has it: their number, the MAE of the pick, the mean
    error bar, and the share with |reference - pick| <= z * bar + slack.  Torch ops where ``horizon`` lives; 4 (S-1) numbers go to
    the host."""
    from metrics import HorizonBars
    S = len(order)
    if horizon.dim() != 3 or horizon.shape[0] != 3 or horizon.shape[1] != S - 1 or seg.dim() != 2 or seg.shape[1] != horizon.shape[2]:
        raise ValueError(f'horizon must be [3, {S - 1}, width] and seg [rows, width] (got {tuple(horizon.shape)} and {tuple(seg.shape)})')
    ref = _reference_boundaries(seg.to(horizon.device), order)
    return HorizonBars(*_bar_sums(horizon, ref, seg.shape[0], z, slack).cpu().numpy(), rows=seg.shape[0], z=z, slack=slack)


def _reference_boundaries(seg, order):
    """The reference's boundaries k = 1 ... S-1 of every column of ``seg`` [rows, width] -> float64 [S-1, width]: the first row
    whose class's position in ``order`` is >= k, ``rows`` where there is none."""
    S, rows = len(order), seg.shape[0]
    pos = torch.full(seg.shape, -1, dtype=torch.int64, device=seg.device)
    for s, k in enumerate(order):
        pos[seg == k] = s
    reached = pos[None] >= torch.arange(1, S, device=seg.device)[:, None, None]                   # [S-1, rows, width]
    return torch.where(reached.any(1), reached.to(torch.int8).argmax(1), rows).to(torch.float64)  # the first such row


def _bar_sums(horizon, ref, rows, z, slack):
    """The four per-boundary sums of `metrics.HorizonBars` for one ``horizon`` [3, S-1, width] against `_reference_boundaries`'
    ``ref`` -> float64 [4, S-1] where ``horizon`` lives."""
    has = ref < rows
    miss = (ref - horizon[0].double()).abs()
    inside = miss <= z * horizon[2].double() + slack
    zero = torch.zeros((), dtype=torch.float64, device=ref.device)
    return torch.stack([has.sum(1).double(), torch.where(has, miss, zero).sum(1), torch.where(has, horizon[2].double(), zero).sum(1),
                        (has & inside).sum(1).double()])


def horizon_bars_sweep(horizon, seg, order, z=2.0, slack=1.0):
    """`horizon_bars` for the G configurations of `segment_sweep(..., posterior=True)` (``horizon`` [G, 3, S-1, width]) -> G
    ``metrics.HorizonBars``: the reference's boundaries are computed ONCE, and all 4 (S-1) G sums go to the host in ONE copy."""
    from metrics import HorizonBars
    S = len(order)
    if horizon.dim() != 4 or horizon.shape[1] != 3 or horizon.shape[2] != S - 1 or seg.dim() != 2 or seg.shape[1] != horizon.shape[3]:
        raise ValueError(f'horizon must be [G, 3, {S - 1}, width] and seg [rows, width] (got {tuple(horizon.shape)} and {tuple(seg.shape)})')
    rows = seg.shape[0]
    ref = _reference_boundaries(seg.to(horizon.device), order)
    host = torch.stack([_bar_sums(h, ref, rows, z, slack) for h in horizon]).cpu().numpy() if horizon.shape[0] else []
    return [HorizonBars(*sums, rows=rows, z=z, slack=slack) for sums in host]


def evaluate_sweep(pred, seg, dataset_id, remove_unc=True, unc_seg=None, nclasses=None):
    """`evaluate` for the G maps of `segment_sweep` (pred [G, rows, cols], int8 on the device as it leaves them) -> G
    ``metrics.Report``: G `crw_hip.confusion` calls queued back to back, ONE copy of all counts to the host at the end.  Same mask
    rules; a label outside 0 ... K-1 that survives the mask in any map raises ``crw_hip.LabelError``."""
    from metrics import Report
    if pred.dim() < 2 or pred[0].numel() != seg.numel():
        raise ValueError(f'pred {tuple(pred.shape)} must be G maps covering the pixels of seg {tuple(seg.shape)}')
    K, seg, mask = _report_rules(pred[0], seg, dataset_id, remove_unc, unc_seg, nclasses)
    host = _host_rows([crw_hip.confusion(seg, p, K, **mask) for p in pred])  # [G, K*K + 2]
    return [Report(row[:K * K].view(K, K), _dropped(row[K * K:], K)) for row in host]


def calibration_sweep(pred, conf, seg, dataset_id, remove_unc=True, unc_seg=None, nclasses=None, bins=10):
    """`calibration` for the G maps of `segment_sweep(..., confidence=kind)` (pred [G, rows, cols], conf [G, rows, cols]) -> G
    ``metrics.Calibration``: G `crw_hip.calibration` calls queued back to back, ONE copy of all histograms to the host at the end,
    like `evaluate_sweep`.  Same mask rules; a label outside 0 ... K-1 that survives the mask in any map raises
    ``crw_hip.LabelError``."""
    if pred.dim() < 2 or pred[0].numel() != seg.numel():
        raise ValueError(f'pred {tuple(pred.shape)} must be G maps covering the pixels of seg {tuple(seg.shape)}')
    K, seg, mask = _report_rules(pred[0], seg, dataset_id, remove_unc, unc_seg, nclasses)
    if conf.shape[0] != pred.shape[0] or conf.numel() != pred.numel():
        raise ValueError(f'conf {tuple(conf.shape)} and pred {tuple(pred.shape)} must cover the same pixels')
    conf = conf.to(pred.device)
    outs = [crw_hip.calibration(seg, p, c, K, bins=bins, **mask) for p, c in zip(pred, conf)]
    host = _host_rows([(n, s.view(torch.int64), d) for n, s, d in outs])  # [G, 3 * bins + 3]
    return [_calibration_of(row, outs[0][1].numel(), K) for row in host]


def _map2d(t, like):
    """`t` as a [rows, cols] map of `like`'s shape (a flat or batched-by-one tensor is viewed, a window stays a window)."""
    return t if t.dim() == 2 else t.reshape(like.shape[-2:])


def horizons(pred, seg, dataset_id, remove_unc=True, unc_seg=None, nclasses=None, min_run=1, tol=2, want_picks=False,
             row_spacing=1.0, unit='rows'):
    """Where are the interfaces, and how thick are the layers?  Per class, the horizon and thickness errors of the label map
    ``pred`` ([rows, cols]) against ``seg`` -> ``metrics.Horizons`` (with ``want_picks``: also the picks, int32 [2, 3, K, cols] on
    pred's device: map (0 seg, 1 pred) x (top, bottom, count)).  `evaluate`'s arguments and mask rules, passed through as
    arguments of the one ``crw_hip.horizons`` call: the pixels it sees are the pixels `evaluate` counts.  ``min_run``: the
    shortest run of equal labels down a column that counts as a layer (1: any pixel); ``tol``: the rows within which a pick counts
    as right.  A surviving label outside 0 ... K-1 raises ``crw_hip.LabelError``."""
    K, seg, mask = _report_rules(pred, seg, dataset_id, remove_unc, unc_seg, nclasses)
    if pred.dim() != 2:
        raise ValueError(f'pred must be a [rows, cols] map (got shape {tuple(pred.shape)})')
    mask = {k: (_map2d(v, pred) if torch.is_tensor(v) else v) for k, v in mask.items()}
    out = crw_hip.horizons(_map2d(seg, pred), pred, K, min_run=min_run, tol=tol, want_picks=want_picks, **mask)
    host = torch.cat([out[0].reshape(-1), out[1]]).cpu()  # the one copy: 18 K + 2 integers
    hz = _horizons_of(host, K, pred.shape, min_run, tol, row_spacing, unit)
    return (hz, out[2]) if want_picks else hz


def horizons_sweep(pred, seg, dataset_id, remove_unc=True, unc_seg=None, nclasses=None, min_run=1, tol=2, row_spacing=1.0,
                   unit='rows'):
    """`horizons` for the G maps of `segment_sweep` (pred [G, rows, cols]) -> G ``metrics.Horizons``: G `crw_hip.horizons` calls
    queued back to back, ONE copy of all statistics to the host at the end, like `evaluate_sweep`.  Same mask rules; a label
    outside 0 ... K-1 that survives the mask in any map raises ``crw_hip.LabelError``."""
    if pred.dim() != 3 or pred[0].numel() != seg.numel():
        raise ValueError(f'pred {tuple(pred.shape)} must be G [rows, cols] maps covering the pixels of seg {tuple(seg.shape)}')
    K, seg, mask = _report_rules(pred[0], seg, dataset_id, remove_unc, unc_seg, nclasses)
    mask = {k: (_map2d(v, pred) if torch.is_tensor(v) else v) for k, v in mask.items()}
    seg = _map2d(seg, pred)
    host = _host_rows([crw_hip.horizons(seg, p, K, min_run=min_run, tol=tol, **mask) for p in pred])  # [G, 18 K + 2]
    return [_horizons_of(row, K, pred.shape[1:], min_run, tol, row_spacing, unit) for row in host]


def labelled_columns(n_cols, seq_length, patch_size, overlap, use_last, anchor_cols=(), seeds=True):
    """Which pixel columns of `segment`'s map were labelled, by `_segment_passes`'s arithmetic -> (labelled, segments, direction,
    step) for `label_reach`.  ``n_cols``: the reference map's columns (the result map has the whole items' n_rg * rg_len of them:
    segments[-1]).  Every item (rg_len = T * (W - ow) + ow columns, one segment) is seeded from the W pixel columns of its first
    frame; with ``use_last`` the reverse pass seeds it from those of its last frame as well and the labels travel in both
    directions ('both'), otherwise 'forward'; an anchored pixel column labels every pixel column of its frame
    (`utils.anchor_nodes`: frame min(x mod rg_len // (W - ow), T - 1)).  step = W - ow pixel columns per frame.  The traces of a
    memory bank are labelled elsewhere and are no positions in this map: for a ``seedless`` run pass seeds=False, which leaves the
    anchors alone -- an item without any then falls into the unreached group."""
    T, (H, W), (oh, ow) = int(seq_length), patch_size, overlap
    step = W - ow
    rg_len = T * step + ow
    n_rg = int(n_cols) // rg_len
    if n_rg < 1:
        raise ValueError(f"{n_cols} columns hold no item of {rg_len} columns")
    labelled = set()
    for t in range(n_rg if seeds else 0):
        labelled.update(range(rg_len * t, rg_len * t + W))
        if use_last:
            labelled.update(range(rg_len * (t + 1) - W, rg_len * (t + 1)))
    for x in sorted(int(c) for c in anchor_cols):
        if not 0 <= x < n_rg * rg_len:
            raise ValueError(f"anchored column {x} lies outside the {n_rg} item(s) of {rg_len} columns")
        a = x // rg_len * rg_len + min(x % rg_len // step, T - 1) * step
        labelled.update(range(a, a + W))
    return sorted(labelled), [rg_len * t for t in range(n_rg + 1)], 'both' if use_last else 'forward', step


def _reach_groups(pred, labelled, step, segments, direction, edges):
    """The column groups of `label_reach` for maps of pred's width -> (group map on pred's device, number of groups, edges, the
    largest frame distance of every group's columns: -1 for a group without columns)."""
    group, frames = crw_hip.column_groups(pred.shape[-1], labelled, step, edges=edges, segments=segments, direction=direction)
    edges = list(crw_hip.REACH_EDGES if edges is None else edges)
    groups = len(edges) + 2
    last = torch.full((groups,), -1, dtype=torch.int64).scatter_reduce(0, group.to(torch.int64), frames, 'amax', include_self=True)
    return group.to(pred.device), groups, edges, last


def _reach_of(row, groups, K, has_conf, edges, last):
    """A host row of `crw_hip.confusion_grouped`'s outputs (counts [groups, K, K], the bit pattern of conf_sum [groups] when there
    is a confidence map, dropped [4])."""
    from metrics import Reach
    n = groups * K * K
    conf_sum = row[n:n + groups].view(torch.float64) if has_conf else None
    return Reach(row[:n].view(groups, K, K), conf_sum, _dropped(row[n + groups * has_conf:], K), edges=edges, last_frame=last)


def _reach_maps(pred, seg, conf, mask):
    if pred.dim() != 2:
        raise ValueError(f'pred must be a [rows, cols] map (got shape {tuple(pred.shape)})')
    if conf is not None and conf.numel() != pred.numel():
        raise ValueError(f'conf {tuple(conf.shape)} and pred {tuple(pred.shape)} must cover the same pixels')
    mask = {k: (_map2d(v, pred) if torch.is_tensor(v) else v) for k, v in mask.items()}
    return _map2d(seg, pred), None if conf is None else _map2d(conf.to(pred.device), pred), mask


def label_reach(pred, seg, dataset_id, labelled, step, segments=None, direction='both', edges=None, conf=None, remove_unc=True,
                unc_seg=None, nclasses=None):
    """How far do the labels travel?  The accuracy of the label map ``pred`` ([rows, cols]) against ``seg``, binned by the distance
    of every column, in frames of ``step`` pixel columns, from the nearest labelled column of its own item -> ``metrics.Reach``.
    ``labelled``, ``segments``, ``direction``, ``step``: what `labelled_columns` returns for a `segment` call, or a caller's own
    (`crw_hip.column_groups` has the definition and ``edges``).  ``conf``: the map's confidences, for the mean confidence per
    group.  `evaluate`'s arguments and mask rules, passed through as arguments of the one ``crw_hip.confusion_grouped`` call: the
    pixels it counts are the pixels `evaluate` counts.  A surviving label outside 0 ... K-1 raises ``crw_hip.LabelError``; a
    surviving confidence that is NaN or outside [0, 1] is counted in ``dropped[2]`` and in no group."""
    K, seg, mask = _report_rules(pred, seg, dataset_id, remove_unc, unc_seg, nclasses)
    seg, conf, mask = _reach_maps(pred, seg, conf, mask)
    group, groups, edges, last = _reach_groups(pred, labelled, step, segments, direction, edges)
    counts, conf_sum, dropped = crw_hip.confusion_grouped(seg, pred, K, group, groups, conf=conf, **mask)
    parts = [counts.reshape(-1)] + ([conf_sum.view(torch.int64)] if conf is not None else []) + [dropped]
    return _reach_of(torch.cat(parts).cpu(), groups, K, conf is not None, edges, last)  # the one copy


def label_reach_sweep(pred, seg, dataset_id, labelled, step, segments=None, direction='both', edges=None, conf=None, remove_unc=True,
                      unc_seg=None, nclasses=None):
    """`label_reach` for the G maps of `segment_sweep` (pred [G, rows, cols], conf [G, rows, cols] or None) -> G ``metrics.Reach``:
    one group map, G `crw_hip.confusion_grouped` calls queued back to back, ONE copy of all counts to the host at the end, like
    `evaluate_sweep`.  Same mask rules; a label outside 0 ... K-1 that survives the mask in any map raises ``crw_hip.LabelError``."""
    if pred.dim() != 3 or pred[0].numel() != seg.numel():
        raise ValueError(f'pred {tuple(pred.shape)} must be G [rows, cols] maps covering the pixels of seg {tuple(seg.shape)}')
    if conf is not None and (conf.shape[0] != pred.shape[0] or conf.numel() != pred.numel()):
        raise ValueError(f'conf {tuple(conf.shape)} and pred {tuple(pred.shape)} must cover the same pixels')
    K, seg, mask = _report_rules(pred[0], seg, dataset_id, remove_unc, unc_seg, nclasses)
    seg, _, mask = _reach_maps(pred[0], seg, None, mask)
    group, groups, edges, last = _reach_groups(pred, labelled, step, segments, direction, edges)
    confs = [None] * pred.shape[0] if conf is None else conf.to(pred.device)
    outs = [crw_hip.confusion_grouped(seg, p, K, group, groups, conf=c, **mask) for p, c in zip(pred, confs)]
    host = _host_rows([(n,) + ((s.view(torch.int64),) if s is not None else ()) + (d,) for n, s, d in outs])
    return [_reach_of(row, groups, K, conf is not None, edges, last) for row in host]


# the reference's three per-dataset drivers (scripts/test/test_mc1.py:19-30, test_mc3.py:19-33, test_sharad.py:19-32): argparse
# defaults, the class count and encoder they hard-code, and the change points test_mc3 / test_sharad set by hand before correcting
DRIVERS = {
    'mc1': dict(patch_size=(32, 32), seq_length=100, overlap=(24, 0), cxt_size=80, radius=30, temp=0.1, knn=20, nclasses=4,
                model=1, use_last=True, correction=False, change_idx=None, outputs=('mc1_res.pt',)),
    'mc3': dict(patch_size=(32, 32), seq_length=100, overlap=(30, 0), cxt_size=100, radius=60, temp=0.01, knn=20, nclasses=5,
                model=1, use_last=True, correction=True, change_idx=(38, 36, 52),
                outputs=('mc3_res.pt', 'mc3_resy.pt', 'mc3_xenty.pt')),
    'sharad': dict(patch_size=(16, 16), seq_length=100, overlap=(8, 0), cxt_size=100, radius=10, temp=0.1, knn=20, nclasses=5,
                   model=1, use_last=True, correction=True, change_idx=(80, 67, 98), outputs=('s_res.pt', 's_xent.pt')),
}


def _items(rg, patch_size, overlap):
    """[rows, cols] radargram -> [T, N, H, W]: every patch of the radargram, one item (test_mc1.py:68-72)."""
    (H, W), (OH, OW) = patch_size, overlap
    return rg.unfold(0, H, H - OH).unfold(1, W, W - OW).permute(1, 0, 2, 3)


@torch.no_grad()
def segment_radargrams(driver, radargrams, refs, encoder, refs_reversed=None, patch_size=None, seq_length=None, overlap=None,
                       cxt_size=None, radius=None, temp=None, knn=None, use_last=None, correction=None, change_idx=None, lp=None,
                       context=None):
    """``main(args)`` of the reference's scripts/test/test_{mc1,mc3,sharad}.py (``driver``) without the plots.

    radargrams, refs: three [rows, cols] radargrams and their reference segmentations, as the script holds them after loading
    (``scripts/segment_drivers.py`` reads its files, casts and edits); refs_reversed: mc1's separate references of the reversed
    radargrams.  Every other argument defaults to ``DRIVERS[driver]``; ``lp``: a label-propagation object (default
    ``LabelPropVOS_CRW`` on the driver's CXT_SIZE / RADIUS / TEMP / KNN); ``context``: that object's CONTEXT ('reference', the
    default and what the scripts compute, or 'sliding': labels from the frames the scores were taken on).
    -> {output file name: object}, what the script passes to ``torch.save``, in the state it has at that call.

    Operation for operation, which includes:
      * every radargram is ONE item, ``unfold(0, H, H-OH).unfold(1, W, W-OW).permute(1,0,2,3)``; ``T``, ``N``, ``rg_len`` and
        ``rg_h`` are those of radargram 0 and serve all three, and maps are upsampled (nearest) to ``(rg_h, rg_len)`` -- not to
        the reference segmentation's row count;
      * the forward pass seeds from ``ref[:rg_h, :W]`` (mc1 :98, mc3 :97, sharad :96); ``propagate`` still computes its change
        point, which mc1 ignores and mc3 / sharad overwrite with hand-set ones (``change_idx``, mc3 :111-113, sharad :112-114);
      * correction (mc3 only when ``correction`` is set, sharad always; mc1 never): the item is the TAIL ``rg[t][change_idx:]`` --
        unlike test_all.py's ``get_smaller_item``, which takes the head --, ``px = (seq_length - change_idx) * (W - OW)`` with the
        ``seq_length`` argument, not ``T``, the seed ``ref[:, rg_len-px : rg_len-px+W]`` over ALL rows, and the result resized to
        ``(rg_h, px)`` into the last ``px`` columns; nothing is caught, an error ends the run (mc3 :116-132, sharad :118-129);
      * reverse pass (mc1 / mc3 with ``use_last``; sharad declares the flag and never reads it): mc1 seeds from the reversed
        reference ``refs_reversed[t][:rg_h, :W]`` (:110-122), mc3 from ``ref[:rg_h, -W:]`` (:136-148); ``use_last=True``, the map
        flipped along its columns;
      * merge, in place on the forward (mc3: corrected) maps as the scripts' list aliasing does: mc1 writes 2 where the reverse
        map is 2, then 1 where it is 1 and the ALREADY UPDATED forward map is not 2 (:124-135); mc3 writes 2 where the reverse
        map is 2 and the forward column holds no class 4, then 3 the same way (:150-160);
      * outputs: mc1 ``mc1_res.pt`` (the merged maps); mc3 ``mc3_res.pt`` (the corrected maps as saved BEFORE the merge mutates
        them), ``mc3_resy.pt`` (merged), ``mc3_xenty.pt`` (the forward passes' metric); sharad ``s_res.pt``, ``s_xent.pt``.
        mc1 and mc3 without the reverse pass end in a NameError in the reference (the merged list is never made): refused here."""
    from imported.labelprop import LabelPropVOS_CRW
    if driver not in DRIVERS:
        raise ValueError(f'unknown driver {driver!r} (one of {", ".join(DRIVERS)})')
    d = DRIVERS[driver]
    pick = lambda v, k: d[k] if v is None else v
    patch_size, overlap = tuple(pick(patch_size, 'patch_size')), tuple(pick(overlap, 'overlap'))
    seq_length, nclasses = pick(seq_length, 'seq_length'), d['nclasses']
    use_last, correction = pick(use_last, 'use_last'), pick(correction, 'correction')
    change_idx = pick(change_idx, 'change_idx')
    if len(radargrams) != 3 or len(refs) != 3:
        raise ValueError('the drivers segment exactly three radargrams')
    if driver == 'mc1' and (refs_reversed is None or len(refs_reversed) != 3):
        raise ValueError('mc1 seeds its reverse pass from three reversed references (refs_reversed)')
    if driver in ('mc1', 'mc3') and not use_last:
        raise ValueError(f'{driver}: the reference saves its maps only after the reverse pass (use_last)')
    if driver != 'mc1' and (change_idx is None or len(change_idx) != 3):
        raise ValueError(f'{driver}: three hand-set change points are needed (change_idx)')
    if lp is None:
        lp = LabelPropVOS_CRW(dict(CXT_SIZE=pick(cxt_size, 'cxt_size'), RADIUS=pick(radius, 'radius'), TEMP=pick(temp, 'temp'),
                                   KNN=pick(knn, 'knn'), CONTEXT='reference' if context is None else context))
    OW = overlap[-1]
    rg = [_items(r, patch_size, overlap) for r in radargrams]
    T, N, H, W = rg[0].shape
    rg_len = T * (W - OW) + OW
    rg_h = N * (H - overlap[0]) + overlap[0]

    maps, xents = [], []
    for t in range(3):
        pred, xent, _ = propagate(rg[t], refs[t][:rg_h, :W], encoder, lp, nclasses, False, use_last=False)
        maps.append(_upsample(pred, rg_h, rg_len))
        xents.append(xent)

    if driver == 'sharad' or (driver == 'mc3' and correction):
        for t, ci in enumerate(change_idx):
            if ci is None:
                continue
            px = (seq_length - ci) * (patch_size[-1] - OW)
            seg_ref = refs[t][:, rg_len - px:rg_len - px + W]
            pred, _, _ = propagate(rg[t][ci:], seg_ref, encoder, lp, nclasses, False, use_last=False)
            maps[t][:, rg_len - px:] = _upsample(pred, rg_h, px)

    if driver == 'sharad':
        return {'s_res.pt': maps, 's_xent.pt': xents}
    saved = [m.clone() for m in maps] if driver == 'mc3' else None  # torch.save writes mc3_res.pt before the merge mutates the maps

    rev = []
    for t in range(3):
        seg_ref = refs_reversed[t][:rg_h, :W] if driver == 'mc1' else refs[t][:rg_h, -W:]
        pred, _, _ = propagate(rg[t], seg_ref, encoder, lp, nclasses, False, use_last=True)
        rev.append(torch.flip(_upsample(pred, rg_h, rg_len), (-1,)))
    merge = merge_mc1 if driver == 'mc1' else merge_mc3
    for t in range(3):
        merge(maps[t], rev[t])
    if driver == 'mc1':
        return {'mc1_res.pt': maps}
    return {'mc3_res.pt': saved, 'mc3_resy.pt': maps, 'mc3_xenty.pt': xents}


def merge_mc1(fwd, rev):
    """test_mc1.py:129-133, in place on ``fwd``: class 2 of the reverse map wins; then class 1 wherever ``fwd`` -- already
    updated by the first write -- is not 2."""
    fwd[rev == 2] = 2
    fwd[torch.logical_and(rev == 1, fwd != 2)] = 1
    return fwd


def merge_mc3(fwd, rev):
    """test_mc3.py:155-158, in place on ``fwd``: classes 2, then 3, of the reverse map win in the columns of ``fwd`` that hold
    no class 4."""
    rows = fwd.shape[0]
    for c in (2, 3):
        fwd[torch.logical_and(rev == c, torch.all(fwd != 4, dim=0)[None].repeat(rows, 1))] = c
    return fwd
