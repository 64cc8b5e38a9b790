"""k-NN label propagation (``LabelPropVOS_CRW``) -- same ``cfg`` keys and ``predict`` signature as
the reference (src/imported/labelprop.py:42-115, which in turn follows videowalk, Jabri et al.
2020), computed by the HIP kernels ``crw_labelprop_topk`` / ``crw_labelprop_gather``.

Two entry points:
  * ``predict(feats, masks, curr_feat)`` -- the reference's frame-at-a-time interface;
  * ``propagate_all(feats, seed, nclasses)`` -- whole radargram in two launches (what
    ``utils.propagate`` uses): affinities/top-k of every frame at once, then one sequential
    gather kernel.  Both produce identical label maps.

Optional ``cfg['CONTEXT']``: ``'reference'`` (the default: the reference's rule, its index quirk included) or ``'sliding'`` -- once a
frame lies more than CXT_SIZE + 1 frames into the item, its neighbours' labels are taken from the frames the scores were taken on
(frame 0 and the last CXT_SIZE frames), as upstream videowalk does (``crw_labelprop_propagate_sliding``).

``LabelPropSweep`` is ``propagate_all`` for a whole grid of (RADIUS, TEMP, KNN) settings on the same features -- the grid of the
reference's scripts/launch/launch_test_batch.sh -- sharing what does not depend on the setting.
"""
import os

import torch

import crw_hip

MASK_NEG = -1e10
ANCHORS_NEED_SLIDING = ("anchors need CONTEXT 'sliding': under the reference's index quirk a frame beyond CXT_SIZE + 1 never reads a "
                        "label later than frame CXT_SIZE, so an anchor there would change only itself")


MEMORY_NEEDS_SLIDING = ("memory needs CONTEXT 'sliding': under the reference's index quirk a frame beyond CXT_SIZE + 1 never reads a "
                        "label later than frame CXT_SIZE, so it would not read the bank's rows consistently")


def check_memory(memory, N, nclasses, context, anchor_context='clamp'):
    """The option checks of `memory=` (mem_feats [B, N, C] normalised features, mem_labels [B, N] class ids of B fully labelled
    traces) -> (mem_feats, mem_labels int64)."""
    if context != 'sliding':
        raise ValueError(MEMORY_NEEDS_SLIDING)
    if anchor_context != 'clamp':
        raise ValueError("memory and anchor_context='restart' are not combined: a restart drops every long-term frame but its origin")
    mem_feats, mem_labels = memory
    if mem_feats.dim() != 3 or mem_feats.shape[0] < 1 or tuple(mem_labels.shape) != tuple(mem_feats.shape[:2]):
        raise ValueError(f"memory must be (features [B >= 1, N, C], labels [B, N]) (got {tuple(mem_feats.shape)}, {tuple(mem_labels.shape)})")
    if mem_feats.shape[1] != N:
        raise ValueError(f"the bank's traces have {mem_feats.shape[1]} nodes, the item's {N}: a bank serves items of its own N")
    labels = mem_labels.to(torch.int64)
    if bool(((labels < 0) | (labels >= nclasses)).any()):
        raise ValueError(f"the bank's traces must be fully labelled with classes in [0, {nclasses})")
    return mem_feats, labels


def restart_origin(anchor_context, anchors, context, T, N, nclasses):
    """The option checks of `anchor_context=` -> the origin array of 'restart' (`crw_hip.anchor_origins`; row 0 of the anchors is
    the seed's and restarts nothing more than frame 0 does), None under 'clamp'."""
    if crw_hip.check_anchor_context(anchor_context) == 'clamp':
        return None
    if anchors is None:
        raise ValueError("anchor_context='restart' needs anchors: a restart happens at a fully anchored frame")
    if context != 'sliding':
        raise ValueError(ANCHORS_NEED_SLIDING)
    crw_hip.check_anchors(anchors, T, N, nclasses)
    return crw_hip.anchor_origins(anchors, nclasses, T)


class LabelPropVOS_CRW(object):
    def __init__(self, cfg):
        self.cxt_size = cfg['CXT_SIZE']
        self.radius = cfg['RADIUS']
        self.temperature = cfg['TEMP']
        self.topk = cfg['KNN']
        # optional: which frames an index of a late frame (n > CXT_SIZE + 1) addresses -- 'reference': the untruncated label list,
        # as the reference does (quirk Q7); 'sliding': the frames the scores were taken on (upstream videowalk's rule)
        self.context = cfg.get('CONTEXT', 'reference')
        if self.context not in crw_hip.CONTEXTS:
            raise ValueError(f"cfg['CONTEXT'] must be one of {crw_hip.CONTEXTS} (got {self.context!r})")
        self.mask = None
        self.mask_hw = None

    # context bookkeeping of the videowalk interface (kept for API compatibility)
    def context_long(self, t0, t):
        return [t0]

    def context_short(self, t0, t):
        return [max(tt, t0) for tt in range(t - self.cxt_size, t)]

    def context_index(self, t0, t):
        return self.context_long(t0, t) + self.context_short(t0, t)

    def _band(self, h, w, dev):
        """additive locality mask [1, h*w, h*w]: 0 inside the radius, -1e10 outside.  Kept as an
        attribute like the reference; the kernels apply the same band arithmetically."""
        if self.mask is None or self.mask_hw != (h, w):
            i = torch.arange(h, device=dev).repeat_interleave(w).float()
            j = torch.arange(w, device=dev).repeat(h).float()
            d = ((i[:, None] - i[None, :]) ** 2 + (j[:, None] - j[None, :]) ** 2).sqrt()
            self.mask = torch.where(d < self.radius, 0.0, MASK_NEG)[None]
            self.mask_hw = (h, w)
        return self.mask

    def _check_grid(self, h, w):
        if self.topk > h * w:
            raise RuntimeError(f"KNN={self.topk} exceeds the number of nodes per frame ({h * w}); "
                               "torch.topk in the reference raises for the first frame as well")

    def predict(self, feats, masks, curr_feat, ref_index=None, t=None):
        """feats: list of n [1,C,h,w] context features; masks: list of n [1,M,h,w] soft labels;
        curr_feat [1,C,h,w]  ->  soft labels of the current frame [1,M,h,w].  A radargram's frames are columns of patches
        (w = 1, what `utils.propagate` passes); any h x w grid is taken like the reference's (nodes in row-major order, the band
        the Euclidean disc of `MaskedAttention`, src/imported/maskedatt.py:222-245).
        CONTEXT 'sliding': handed more than CXT_SIZE + 1 frames, the result is what the reference's `predict` returns on the
        windowed lists `[feats[0]] + feats[-CXT_SIZE:]` (masks likewise)."""
        h, w = curr_feat.shape[-2:]
        self._check_grid(h, w)
        self._band(h, w, curr_feat.device)
        n, N = len(feats), h * w
        E = torch.cat(list(feats) + [curr_feat], 0).flatten(2).permute(0, 2, 1).contiguous().float()  # [n+1, N, C]
        M = masks[0].shape[1]
        L = torch.empty((n + 1) * N, M, device=E.device, dtype=torch.float32)
        L[:n * N] = torch.cat(list(masks), 0).flatten(2).permute(0, 2, 1).reshape(n * N, M)
        Wt, It = crw_hip.labelprop_topk(E, self.cxt_size, self.radius, self.temperature, self.topk, first_frame=n, grid_w=w)
        crw_hip.labelprop_gather(None, Wt, It, n + 1, N, M, first_frame=n, L=L, cxt_size=self.cxt_size, context=self.context)
        return L[n * N:].reshape(N, M).t().reshape(1, M, h, w)

    def _propagate_memory(self, feats, seed, nclasses, grid_w, anchors, anchor_context, memory, memory_bias=0.0):
        """`propagate_all(memory=)`: the virtual item [bank traces..., item], the bank's B frames (and the item's frame 0 when it is
        seeded) long-term -- crw_labelprop_topk_long / crw_labelprop_propagate_long through `crw_hip.labelprop_topk(n_long=)` and
        `labelprop_gather(n_long=)`.  The rows in front are one-hot; the item's part of pred and L is returned.
        memory_bias other than 0: the lists are crw_labelprop_topk_long_bias's (`labelprop_topk(long_bias=)`)."""
        T, N, C = feats.shape
        bias = crw_hip.check_memory_bias(memory_bias)
        mem_feats, labels = check_memory(memory, N, nclasses, self.context, anchor_context)
        if grid_w != 1:
            raise ValueError("memory is defined on N x 1 grids only")
        B = mem_feats.shape[0]
        front = labels if seed is None else torch.cat([labels, seed.to(labels.device).long()[None]])
        K, F = front.shape[0], B + T
        ehat = torch.cat([mem_feats.to(feats.dtype), feats]).contiguous()
        self._check_grid(N, 1)
        bkw = dict(long_bias=bias) if bias != 0.0 else {}   # 0: the call as it is without the option
        Wt, It = crw_hip.labelprop_topk(ehat, self.cxt_size, self.radius, self.temperature, self.topk, first_frame=K, n_long=K, route="auto", **bkw)
        if anchors is not None:
            crw_hip.check_anchors(anchors, T, N, nclasses)
            shifted = torch.cat([torch.full((B, N), -1, dtype=torch.int8, device=anchors.device), anchors])   # B frames further down
            crw_hip.mark_anchors(Wt, It, shifted, nclasses, K)
        L = torch.empty(F * N, nclasses, device=feats.device, dtype=torch.float32)
        pred = torch.zeros(N, F, device=feats.device, dtype=torch.float32)
        front = front.to(feats.device)
        L[:K * N] = (front.reshape(-1, 1) == torch.arange(nclasses, device=feats.device)).to(L.dtype)
        pred[:, :K] = front.t().to(pred.dtype)
        crw_hip.labelprop_gather(None, Wt, It, F, N, nclasses, first_frame=K, L=L, pred=pred, cxt_size=self.cxt_size, context='sliding',
                                 n_long=K, route="auto")
        return pred[:, B:].contiguous(), L[B * N:]

    def propagate_all(self, feats, seed, nclasses, grid_w=1, anchors=None, anchor_context='clamp', memory=None, memory_bias=0.0):
        """feats [T,N,C] (normalised features), seed [N] float class ids of frame 0
        -> (pred [N,T] float class ids, L [T*N, M] soft labels).  grid_w: the N nodes are an (N / grid_w) x grid_w grid.
        memory (needs CONTEXT 'sliding', anchor_context 'clamp', an N x 1 grid): (mem_feats [B, N, C], mem_labels [B, N]) -- B fully
        labelled traces from elsewhere (another item, another radargram), normalised features of the same encoder.  They are put in
        front of the item as long-term frames: every frame scores against them and against its CXT_SIZE predecessors, and reads
        their labels (include/crw_hip_longmem.h).  With a seed the item's frame 0 is one more long-term frame; seed=None (memory
        only): the item's frame 0 is predicted from the bank alone and is an ordinary frame afterwards.  Anchors move B frames down
        with the item.  The item's pred [N,T] and L [T*N, M] are returned, nothing of the bank's.  None: the call is what it was.
        memory_bias (needs memory; a finite float, default 0.0: nothing changes): added to the cosine of every in-band key of the
        long-term frames -- the bank's and, with a seed, the item's frame 0 -- before the division by the temperature
        (include/crw_hip_align.h), so that a long-term key b closer than it scores wins a slot against a recent key.
        anchor_context 'restart' (needs anchors): a frame whose N nodes are all anchored is as good as a seed -- every frame behind
        it is propagated as a frame of the item that starts there (`crw_hip.anchor_origins`, the `origin=` of `labelprop_topk` and
        `labelprop_gather`); 'clamp': the anchors clamp and the context is what it is without them.
        anchors (needs CONTEXT 'sliding'): [T, N] int8, device or host, labelled nodes inside the item -- a class id in [0, nclasses)
        clamps the node's soft labels to that class before the next frame reads them, anything else (-1) leaves the node free; row 0
        is ignored (the seed rules there).  The lists made here are this call's own, so the anchors are marked into them in place
        (`crw_hip.mark_anchors`, no copy) and ONE crw_labelprop_propagate_sliding call follows; CRW_ANCHORS_SEGMENTED=1 (read per call)
        or a library without the marks: one launch per stretch between anchored frames (`crw_hip.labelprop_gather(anchors=)`)."""
        T, N, C = feats.shape
        if memory is not None:
            return self._propagate_memory(feats, seed, nclasses, grid_w, anchors, anchor_context, memory, memory_bias)
        if crw_hip.check_memory_bias(memory_bias) != 0.0:
            raise ValueError("memory_bias needs memory: without a bank the long-term part of a list is the seed frame alone")
        if seed is None:
            raise ValueError("seed=None needs memory: without a bank nothing labels the item's first frame")
        origin = restart_origin(anchor_context, anchors, self.context, T, N, nclasses)
        if anchors is not None and self.context != 'sliding':
            raise ValueError(ANCHORS_NEED_SLIDING)
        self._check_grid(N // grid_w, grid_w)
        self._band(N // grid_w, grid_w, feats.device)
        Wt, It = crw_hip.labelprop_topk(feats, self.cxt_size, self.radius, self.temperature, self.topk, first_frame=1, grid_w=grid_w,
                                        origin=origin)
        kw = {} if origin is None else dict(origin=origin)
        if anchors is not None:
            crw_hip.check_anchors(anchors, T, N, nclasses)
            if origin is None and crw_hip.anchors_segmented():
                kw = dict(anchors=anchors)
            else:
                crw_hip.mark_anchors(Wt, It, anchors, nclasses, 1)
        L, pred = crw_hip.labelprop_gather(seed.float().contiguous(), Wt, It, T, N, nclasses, first_frame=1, cxt_size=self.cxt_size,
                                           context=self.context, **kw)
        return pred, L

    def novelty(self, feats, anchors=None, anchor_context='clamp', top=None, nclasses=None):
        """feats [T,N,C] (normalised features, a column of patches) -> (nov [T-1, N], score [T-1]) of frames 1 .. T-1 on the device:
        how little each node's best key in this propagation's context resembles it, and the mean of each frame's `top` (default
        max(1, N // 4)) largest (`crw_hip.labelprop_novelty`; RADIUS and CXT_SIZE are this object's, TEMP and KNN play no part).
        anchors / anchor_context as in `propagate_all`: under 'restart' the keys of a frame start at its origin
        (`crw_hip.anchor_origins`; nclasses as there, None: 127, the most that int8 anchors can name), under 'clamp' the anchors change no key.
        `crw_hip.suggest_frames` turns the scores into places to label."""
        T, N, C = feats.shape
        origin = restart_origin(anchor_context, anchors, self.context, T, N, 127 if nclasses is None else nclasses)
        return crw_hip.labelprop_novelty(feats, self.cxt_size, self.radius, top=top, first_frame=1, origin=origin)


class LabelPropSweep(object):
    """Label propagation for every (RADIUS, TEMP, KNN) of a grid at one CXT_SIZE -- scripts/launch/launch_test_batch.sh runs
    test_all.py once per point of such a grid.  ``configs``: the ``cfg`` dicts of ``LabelPropVOS_CRW`` in that script's loop order
    (radius outermost, knn innermost); ``propagate_all`` returns the label map of every configuration, each exactly that of
    ``LabelPropVOS_CRW(configs[g]).propagate_all``."""

    def __init__(self, cxt_size, radii, temps, knns, context='reference', biases=(0.0,)):
        """biases: the values of `LabelPropVOS_CRW.propagate_all`'s memory_bias to sweep -- a fourth grid axis between temp and knn
        (radius outermost, then temp, then bias, knn innermost), for `propagate_all(memory=)`.  Other than (0.0,) every cfg carries
        its MEMORY_BIAS; with the default the dicts are what they were."""
        self.cxt_size = int(cxt_size)
        self.context = crw_hip.check_context(context)
        self.radii, self.temps, self.knns = [int(r) for r in radii], [float(t) for t in temps], [int(k) for k in knns]
        if not (self.radii and self.temps and self.knns):
            raise ValueError("radii, temps and knns must each hold at least one value")
        if min(self.knns) < 1 or len(self.knns) > 16:
            raise ValueError("knns: 1 ... 16 values >= 1")
        self.biases = [crw_hip.check_memory_bias(b) for b in biases]
        if not self.biases:
            raise ValueError("biases must hold at least one value")
        self.configs = [dict(CXT_SIZE=self.cxt_size, RADIUS=r, TEMP=t, KNN=k)
                        for r in self.radii for t in self.temps for b in self.biases for k in self.knns]
        if self.biases != [0.0]:  # (the key is absent without the axis: the dicts are what they were)
            for i, cfg in enumerate(self.configs):
                cfg['MEMORY_BIAS'] = self.biases[i // len(self.knns) % len(self.biases)]
        if self.context != 'reference':  # (the key is absent under the default rule: the dicts are what they were)
            for cfg in self.configs:
                cfg['CONTEXT'] = self.context

    def __len__(self):
        return len(self.configs)

    def _check_grid(self, h, w):
        if max(self.knns) > h * w:
            raise RuntimeError(f"KNN={max(self.knns)} exceeds the number of nodes per frame ({h * w}); "
                               "torch.topk in the reference raises for the first frame as well")

    def _propagate_memory(self, feats, seed, nclasses, grid_w, soft, anchors, anchor_context, memory):
        """`propagate_all(memory=)`: `LabelPropVOS_CRW._propagate_memory`'s virtual item [bank traces..., item] for the whole grid.
        Per (radius, temp, bias) one selection at kmax (`labelprop_topk_scores(n_long=K, long_bias=b)`) and one
        `labelprop_sweep_weights`; the one-hot front rows go to every L[g]; ONE `labelprop_propagate_batch(n_long=K)`."""
        T, N, C = feats.shape
        mem_feats, labels = check_memory(memory, N, nclasses, self.context, anchor_context)
        if grid_w != 1:
            raise ValueError("memory is defined on N x 1 grids only")
        self._check_grid(N, 1)
        if anchors is not None:
            crw_hip.check_anchors(anchors, T, N, nclasses)
        if os.environ.get("CRW_SWEEP_PER_CONFIG") == "1":
            akw = {} if anchors is None else dict(anchors=anchors)
            outs = [LabelPropVOS_CRW(cfg).propagate_all(feats, seed, nclasses, memory=memory, memory_bias=cfg.get('MEMORY_BIAS', 0.0), **akw)
                    for cfg in self.configs]
            pred = torch.stack([o[0] for o in outs])
            return (pred, torch.stack([o[1] for o in outs])) if soft else pred
        B = mem_feats.shape[0]
        front = labels if seed is None else torch.cat([labels, seed.to(labels.device).long()[None]])
        K, Fv = front.shape[0], B + T
        ehat = torch.cat([mem_feats.to(feats.dtype), feats]).contiguous()
        nk, kmax, F = len(self.knns), max(self.knns), Fv - K
        P = len(self.radii) * len(self.temps) * len(self.biases)
        G = P * nk
        W = torch.empty(P, nk, F, kmax, N, device=feats.device, dtype=torch.float32)
        I = torch.empty(P, F, kmax, N, device=feats.device, dtype=torch.int32)
        V = torch.empty(F, kmax, N, device=feats.device, dtype=torch.float32)
        p = 0
        for r in self.radii:
            for t in self.temps:
                for b in self.biases:
                    bkw = dict(long_bias=b) if b != 0.0 else {}   # 0: the call as it is without the option
                    crw_hip.labelprop_topk_scores(ehat, self.cxt_size, r, t, kmax, first_frame=K, out=(V, I[p]), n_long=K, route="auto", **bkw)
                    crw_hip.labelprop_sweep_weights(V, self.knns, out=W[p])
                    p += 1
        if anchors is not None:  # (a library that has the long-memory entry points honours the marks)
            shifted = torch.cat([torch.full((B, N), -1, dtype=torch.int8, device=anchors.device), anchors])   # B frames further down
            crw_hip.mark_anchors(W.view(G, F, kmax, N), I, shifted, nclasses, K)
        Ig = I[0] if P == 1 else I[:, None].expand(P, nk, F, kmax, N).reshape(G, F, kmax, N)
        L = torch.empty(G, Fv * N, nclasses, device=feats.device, dtype=torch.float32)
        pred = torch.zeros(G, N, Fv, device=feats.device, dtype=torch.float32)
        front = front.to(feats.device)
        L[:, :K * N] = (front.reshape(-1, 1) == torch.arange(nclasses, device=feats.device)).to(L.dtype)
        pred[:, :, :K] = front.t().to(pred.dtype)
        crw_hip.labelprop_propagate_batch(None, W.view(G, F, kmax, N), Ig, Fv, N, nclasses, first_frame=K, cxt_size=self.cxt_size, L=L,
                                          pred=pred, context='sliding', n_long=K)
        pred = pred[:, :, B:].contiguous()
        return (pred, L[:, B * N:].contiguous()) if soft else pred

    def propagate_all(self, feats, seed, nclasses, grid_w=1, soft=False, anchors=None, anchor_context='clamp', memory=None):
        """feats [T,N,C] (normalised features), seed [N] float class ids of frame 0 -> pred [G,N,T] float class ids, G =
        len(configs).  memory (needs context 'sliding', anchor_context 'clamp', an N x 1 grid): `LabelPropVOS_CRW.propagate_all`'s,
        the same bank in front of every configuration; seed may then be None; the biases of the grid are the configurations'
        memory_bias (`_propagate_memory`; crw_labelprop_propagate_long_batch).  anchor_context: `LabelPropVOS_CRW.propagate_all`'s -- under 'restart' ONE origin array serves every selection
        and the batch call (crw_labelprop_propagate_origin_batch).  anchors (needs context 'sliding'): `LabelPropVOS_CRW.propagate_all`'s, the same for every configuration --
        marked in place into the W [G, ...] that `labelprop_sweep_weights` wrote and into the shared I (`crw_hip.mark_anchors`: a
        configuration padded from a smaller knn keeps slot 0 as a real slot), then the ONE batch call as without them.  soft: -> (pred, L [G, T*N, M]), the soft labels of every configuration as well (the batch kernel writes them
        anyway; the per-configuration arm stacks its G copies) -- what `crw_hip.labelmap_dense_batch` turns into pixel maps.

        Per (radius, temp): ONE selection at kcap = max(knns) (`crw_hip.labelprop_topk_scores`; the lists of a smaller knn are
        its first entries) and one `labelprop_sweep_weights` (the softmax of every knn, shorter lists padded with zero weights).
        Then ONE `labelprop_propagate_batch` over all G configurations, a workgroup per configuration (it holds W and I
        [G, T-1, kmax, N] and L [G, T*N, M] at once: 0.3 GB for the 60-point grid at [T, N] = [100, 190]).
        CRW_SWEEP_PER_CONFIG=1 (read per call): a loop of `LabelPropVOS_CRW.propagate_all` over the configurations on the same
        features instead -- the A/B arm of tools/sweep_timing.py, and the fallback."""
        T, N, C = feats.shape
        if memory is not None:
            return self._propagate_memory(feats, seed, nclasses, grid_w, soft, anchors, anchor_context, memory)
        if self.biases != [0.0]:
            raise ValueError("memory_bias needs memory: without a bank the long-term part of a list is the seed frame alone")
        if seed is None:
            raise ValueError("seed=None needs memory: without a bank nothing labels the item's first frame")
        origin = restart_origin(anchor_context, anchors, self.context, T, N, nclasses)
        if anchors is not None:
            if self.context != 'sliding':
                raise ValueError(ANCHORS_NEED_SLIDING)
            crw_hip.check_anchors(anchors, T, N, nclasses)
        self._check_grid(N // grid_w, grid_w)
        seed = seed.float().contiguous()
        if os.environ.get("CRW_SWEEP_PER_CONFIG") == "1":
            akw = {} if anchors is None else dict(anchors=anchors, anchor_context=anchor_context)
            if not soft:
                return torch.stack([LabelPropVOS_CRW(cfg).propagate_all(feats, seed, nclasses, grid_w=grid_w, **akw)[0] for cfg in self.configs])
            outs = [LabelPropVOS_CRW(cfg).propagate_all(feats, seed, nclasses, grid_w=grid_w, **akw) for cfg in self.configs]
            return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
        nk, kmax, F = len(self.knns), max(self.knns), T - 1
        P = len(self.radii) * len(self.temps)
        W = torch.empty(P, nk, F, kmax, N, device=feats.device, dtype=torch.float32)
        I = torch.empty(P, F, kmax, N, device=feats.device, dtype=torch.int32)
        V = torch.empty(F, kmax, N, device=feats.device, dtype=torch.float32)
        p = 0
        for r in self.radii:
            for t in self.temps:
                crw_hip.labelprop_topk_scores(feats, self.cxt_size, r, t, kmax, first_frame=1, grid_w=grid_w, out=(V, I[p]), origin=origin)
                crw_hip.labelprop_sweep_weights(V, self.knns, out=W[p])
                p += 1
        if anchors is not None:  # before I is expanded: every (radius, temp) pair's indices take the classes, every W[g] the marks
            if not crw_hip.has_anchor_lists():
                raise RuntimeError(f"{crw_hip.LIB_PATH} does not honour anchor marks in the lists (a stale libcrw_hip.so): a sweep "
                                   "cannot run as segments -- rebuild with `make -C radar-sounder-crw_amd/csrc`")
            crw_hip.mark_anchors(W.view(P * nk, F, kmax, N), I, anchors, nclasses, 1)
        if P == 1:
            Ig = I[0]  # one list of indices shared by every configuration
        else:
            Ig = I[:, None].expand(P, nk, F, kmax, N).reshape(P * nk, F, kmax, N)  # (a copy: the batch takes one stride)
        L, pred = crw_hip.labelprop_propagate_batch(seed, W.view(P * nk, F, kmax, N), Ig, T, N, nclasses, first_frame=1,
                                                    cxt_size=self.cxt_size, context=self.context, origin=origin)
        return (pred, L) if soft else pred
