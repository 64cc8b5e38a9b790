"""Segmentation reports: what the reference prints at the end of scripts/test/test_all.py (:183-187,
``sklearn.metrics.classification_report`` and ``confusion_matrix``) from ONE [K, K] matrix of counts.

The counts come from ``crw_hip.confusion`` (one pass over the label maps where they are -- the HIP kernel ``crw_confusion`` for
device tensors, ``torch.bincount`` for CPU tensors); a ``Report`` copies those K*K integers to the host once and does the rest in
float64 there.  scikit-learn is not needed; a reference-side script switches with

    from metrics import classification_report, confusion_matrix      # was: from sklearn.metrics import ...

and keeps its code.  sklearn's label semantics are kept, because the fixtures (tests/golden/report_*.npz) come from it: the
reported classes are those that occur in ``gt`` or in ``pred`` (after masking), ascending; a class absent from both has no row,
no column and no share in the macro average; a 0 / 0 ratio is 0.0.  IoU is an addition and is printed by a method of its own
(``iou_str``), so ``str(report)`` stays comparable with sklearn's text character for character.

``Calibration`` is the companion for a confidence map (``inference.segment(..., confidence=kind)['conf']``): the reliability
histogram of ``crw_hip.calibration`` -- per confidence bin, the pixels, the correct pixels and the summed confidence, under the same
masks -- turned into the expected / maximum calibration error and the risk-coverage curve.  The reference has no twin: it marks
"uncertain" pixels with a hand-drawn class (``--remove_unc``).

``Horizons`` reports what a sounder segmentation is used for -- its interfaces: per class, in how many columns the layer was found,
missed or invented, and how far its top, its bottom and its thickness lie from the ground truth's, from the [K, 18] integers of
``crw_hip.horizons``.  No twin in the reference either.
"""
import numpy as np
import torch

import crw_hip


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.zeros(np.broadcast(num, den).shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


class Report:
    """Per-class and averaged scores of a [K, K] count matrix (rows: ground truth, columns: prediction).

    labels (present classes, ascending), matrix [n, n] int64 over those classes, precision / recall / f1 / iou [n] float64,
    support [n] int64, accuracy, macro / weighted (dicts: precision, recall, f1, support), mean_iou, total (= matrix.sum()),
    dropped (masked, invalid) when built by ``inference.evaluate`` / ``from_maps``."""

    def __init__(self, counts, dropped=None, label_type=float):
        if torch.is_tensor(counts):
            counts = counts.detach().cpu().numpy()  # the one device-to-host copy: K*K integers
        full = np.asarray(counts, dtype=np.int64)
        if full.ndim != 2 or full.shape[0] != full.shape[1]:
            raise ValueError(f"counts must be a square matrix (got shape {full.shape})")
        self.counts = full
        self.dropped = None if dropped is None else tuple(int(v) for v in dropped)
        present = np.flatnonzero(full.sum(0) + full.sum(1))
        self.labels = [label_type(i) for i in present]
        self.matrix = full[np.ix_(present, present)]
        tp = np.diag(self.matrix)
        self.support = self.matrix.sum(1)
        predicted = self.matrix.sum(0)
        self.total = int(self.matrix.sum())
        self.precision = _ratio(tp, predicted)
        self.recall = _ratio(tp, self.support)
        self.f1 = _ratio(2 * tp, self.support + predicted)
        self.iou = _ratio(tp, self.support + predicted - tp)
        self.accuracy = float(_ratio(tp.sum(), self.total))
        n = max(len(present), 1)
        w = _ratio(self.support, self.total)
        avg = lambda weights: dict(precision=float((self.precision * weights).sum()), recall=float((self.recall * weights).sum()),
                                   f1=float((self.f1 * weights).sum()), support=self.total)
        self.macro = avg(np.full(len(present), 1.0 / n))
        self.weighted = avg(w)
        self.mean_iou = float(self.iou.sum() / n)

    @classmethod
    def from_maps(cls, gt, pred, K=None, **mask):
        """Counts from two label maps (``crw_hip.confusion``); K defaults to the largest label + 1.  Invalid labels raise."""
        if K is None:
            K = _infer_K(gt, pred)
        counts, dropped = crw_hip.confusion(gt, pred, K, **mask)
        dropped = [int(v) for v in dropped.cpu()]
        if dropped[1]:
            raise crw_hip.LabelError(dropped[1], K)
        return cls(counts, dropped, label_type=float if (torch.is_tensor(gt) and gt.is_floating_point()) else int)

    def as_dict(self):
        """The layout of ``classification_report(..., output_dict=True)`` plus the IoU entries."""
        out = {}
        for i, lab in enumerate(self.labels):
            out[str(lab)] = {"precision": float(self.precision[i]), "recall": float(self.recall[i]), "f1-score": float(self.f1[i]),
                             "support": int(self.support[i]), "iou": float(self.iou[i])}
        out["accuracy"] = self.accuracy
        for name, a in (("macro avg", self.macro), ("weighted avg", self.weighted)):
            out[name] = {"precision": a["precision"], "recall": a["recall"], "f1-score": a["f1"], "support": a["support"]}
        out["mean_iou"] = self.mean_iou
        return out

    def __str__(self, digits=2):
        names = [str(lab) for lab in self.labels]
        width = max([len(n) for n in names] + [len("weighted avg"), digits])
        head = "{:>{w}s} ".format("", w=width) + "".join(" {:>9}".format(h) for h in ("precision", "recall", "f1-score", "support"))
        row = lambda name, p, r, f, s: "{:>{w}s} ".format(name, w=width) + "".join(
            " {:>9.{d}f}".format(v, d=digits) for v in (p, r, f)) + " {:>9}\n".format(s)
        text = head + "\n\n"
        for i, name in enumerate(names):
            text += row(name, self.precision[i], self.recall[i], self.f1[i], int(self.support[i]))
        text += "\n"
        text += "{:>{w}s} ".format("accuracy", w=width) + " {:>9}".format("") * 2 + " {:>9.{d}f} {:>9}\n".format(
            self.accuracy, self.total, d=digits)
        for name, a in (("macro avg", self.macro), ("weighted avg", self.weighted)):
            text += row(name, a["precision"], a["recall"], a["f1"], a["support"])
        return text

    def matrix_str(self):
        return str(self.matrix)

    def iou_str(self, digits=2):
        names = [str(lab) for lab in self.labels]
        width = max([len(n) for n in names] + [len("mean"), digits])
        text = "{:>{w}s}  {:>9}\n\n".format("", "iou", w=width)
        for n, v in zip(names, self.iou):
            text += "{:>{w}s}  {:>9.{d}f}\n".format(n, v, w=width, d=digits)
        return text + "\n{:>{w}s}  {:>9.{d}f}\n".format("mean", self.mean_iou, w=width, d=digits)


class Calibration:
    """Reliability of a confidence map, from the [bins, 2] counts (pixels, correct pixels), the [bins] confidence sums and the
    dropped triple of ``crw_hip.calibration`` (tensors are copied to the host once: 3 * bins + 3 numbers).

    Bin b holds the confidences in [b / bins, (b + 1) / bins) (the last one includes 1).  count / correct [bins] int64, accuracy /
    mean_confidence [bins] float64 (NaN for an empty bin), total, overall accuracy, ece = sum_b count_b / total *
    |accuracy_b - mean_confidence_b|, mce = the largest such gap (both over the non-empty bins; NaN when every bin is empty),
    dropped (masked, invalid label, invalid confidence) or None."""

    def __init__(self, counts, conf_sum, dropped=None):
        host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        counts = np.asarray(host(counts), dtype=np.int64)
        if counts.ndim != 2 or counts.shape[1] != 2 or counts.shape[0] < 1:
            raise ValueError(f"counts must be [bins, 2] (got shape {counts.shape})")
        self.conf_sum = np.asarray(host(conf_sum), dtype=np.float64).reshape(-1)
        if self.conf_sum.shape[0] != counts.shape[0]:
            raise ValueError(f"conf_sum must hold one sum per bin (got {self.conf_sum.shape[0]} for {counts.shape[0]} bins)")
        if (counts < 0).any() or (counts[:, 1] > counts[:, 0]).any():
            raise ValueError("counts must be non-negative with correct <= pixels in every bin")
        self.bins = counts.shape[0]
        self.count, self.correct = counts[:, 0].copy(), counts[:, 1].copy()
        self.dropped = None if dropped is None else tuple(int(v) for v in host(dropped))
        self.total = int(self.count.sum())
        self.edges = np.arange(self.bins + 1, dtype=np.float64) / self.bins
        filled = self.count > 0
        nan = np.full(self.bins, np.nan)
        self.accuracy, self.mean_confidence = nan.copy(), nan.copy()
        np.divide(self.correct, self.count, out=self.accuracy, where=filled)
        np.divide(self.conf_sum, self.count, out=self.mean_confidence, where=filled)
        gap = np.abs(self.accuracy - self.mean_confidence)[filled]
        self.overall_accuracy = float(self.correct.sum() / self.total) if self.total else float("nan")
        self.ece = float((gap * self.count[filled]).sum() / self.total) if self.total else float("nan")
        self.mce = float(gap.max()) if self.total else float("nan")

    def risk_coverage(self):
        """Selective prediction at the thresholds b / bins, b = 0 ... bins - 1: keep the pixels whose confidence is at least the
        threshold -> dict(threshold, coverage, accuracy) of [bins] arrays.  coverage = kept / total never grows with the
        threshold (NaN throughout when no pixel was binned); accuracy of the kept pixels is NaN where none is kept."""
        kept = np.cumsum(self.count[::-1])[::-1].astype(np.float64)
        right = np.cumsum(self.correct[::-1])[::-1].astype(np.float64)
        acc = np.full(self.bins, np.nan)
        np.divide(right, kept, out=acc, where=kept > 0)
        cov = kept / self.total if self.total else np.full(self.bins, np.nan)
        return dict(threshold=self.edges[:-1].copy(), coverage=cov, accuracy=acc)

    @property
    def aurc(self):
        """Area under the risk-coverage curve (risk = 1 - accuracy of the kept pixels): the trapezoid rule over coverage through
        the thresholds that keep at least one pixel, continued from the smallest such coverage down to 0 at that point's risk.
        Lower is better; NaN when no pixel was binned."""
        rc = self.risk_coverage()
        keep = rc["coverage"] > 0
        if not self.total or not keep.any():
            return float("nan")
        cov, risk = rc["coverage"][keep][::-1], 1.0 - rc["accuracy"][keep][::-1]  # coverage ascending
        return float(cov[0] * risk[0] + ((cov[1:] - cov[:-1]) * (risk[1:] + risk[:-1]) / 2).sum())

    def coverage_at(self, accuracy):
        """The largest coverage among the thresholds whose kept pixels reach ``accuracy`` (0.0 when none does)."""
        rc = self.risk_coverage()
        good = rc["accuracy"] >= accuracy  # NaN fails
        return float(rc["coverage"][good].max()) if good.any() else 0.0

    def to_dict(self):
        rc = self.risk_coverage()
        lst = lambda a: [float(v) for v in a]
        d = dict(bins=self.bins, edges=lst(self.edges), count=[int(v) for v in self.count], correct=[int(v) for v in self.correct],
                 accuracy=lst(self.accuracy), mean_confidence=lst(self.mean_confidence), total=self.total,
                 overall_accuracy=self.overall_accuracy, ece=self.ece, mce=self.mce, aurc=self.aurc,
                 risk_coverage=dict(threshold=lst(rc["threshold"]), coverage=lst(rc["coverage"]), accuracy=lst(rc["accuracy"])))
        if self.dropped is not None:
            d["dropped"] = dict(masked=self.dropped[0], invalid=self.dropped[1], invalid_confidence=self.dropped[2])
        return d

    def __str__(self, digits=4):
        rc = self.risk_coverage()
        num = lambda v: "{:>10}".format("-") if v != v else "{:>10.{d}f}".format(v, d=digits)
        text = "{:>13} {:>12} {:>10} {:>10} {:>10} {:>10}\n\n".format("confidence", "pixels", "accuracy", "mean conf", "coverage",
                                                                     "kept acc")
        for b in range(self.bins):
            name = "[{:.3f},{:.3f}{}".format(self.edges[b], self.edges[b + 1], "]" if b == self.bins - 1 else ")")
            text += "{:>13} {:>12} {} {} {} {}\n".format(name, int(self.count[b]), num(self.accuracy[b]), num(self.mean_confidence[b]),
                                                         num(rc["coverage"][b]), num(rc["accuracy"][b]))
        text += "\n"
        for name, v in (("ECE", self.ece), ("MCE", self.mce), ("AURC", self.aurc), ("accuracy", self.overall_accuracy)):
            text += "{:>13} {:>12} {}\n".format(name, self.total if name == "accuracy" else "", num(v))
        return text


class Horizons:
    """Horizon and thickness errors per class, from the [K, 18] statistics and the dropped pair of ``crw_hip.horizons`` (tensors
    are copied to the host once: 18 K + 2 integers).

    n_both / n_missing / n_spurious [K] int64: columns in which both maps, the ground truth only, the prediction only have a
    qualifying run of the class.  presence_precision = n_both / (n_both + n_spurious), presence_recall = n_both / (n_both +
    n_missing), NaN for 0 / 0.  For each quantity q in QUANTITIES ('top', 'bottom', 'thickness'; 'count' reads as 'thickness'),
    over the n_both columns with d = pred - gt: errors[q] = dict(mae, rmse, bias, max: [K] float64 in ``unit`` = rows *
    ``row_spacing``, NaN where n_both = 0; within: the fraction of those columns with |d| <= tol rows), with ``mae(k, q)`` for one
    number.  The integers stay available: ``stats``, and sum_abs / sum_sq / max_abs / n_within / sum_d [q] in rows."""

    QUANTITIES = ("top", "bottom", "thickness")

    def __init__(self, stats, dropped, rows, cols, min_run, tol, row_spacing=1.0, unit="rows"):
        host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        stats = np.asarray(host(stats), dtype=np.int64)
        if stats.ndim != 2 or stats.shape[1] != 18 or stats.shape[0] < 1:
            raise ValueError(f"stats must be [K, 18] (got shape {stats.shape})")
        if (stats[:, :3] < 0).any() or (stats[:, :3].sum(1) > cols).any():
            raise ValueError("n_both + n_missing + n_spurious must lie in 0 ... cols for every class")
        if not row_spacing > 0:
            raise ValueError(f"row_spacing must be positive (got {row_spacing})")
        self.stats, self.K = stats, stats.shape[0]
        self.dropped = None if dropped is None else tuple(int(v) for v in host(dropped))
        self.rows, self.cols, self.min_run, self.tol = int(rows), int(cols), int(min_run), int(tol)
        self.row_spacing, self.unit = float(row_spacing), str(unit)
        self.n_both, self.n_missing, self.n_spurious = stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy()
        nan_ratio = lambda num, den: np.divide(num, den, out=np.full(self.K, np.nan), where=np.asarray(den) != 0)
        self.presence_precision = nan_ratio(self.n_both, self.n_both + self.n_spurious)
        self.presence_recall = nan_ratio(self.n_both, self.n_both + self.n_missing)
        self.sum_abs, self.sum_sq, self.max_abs, self.n_within, self.sum_d = {}, {}, {}, {}, {}
        self.errors = {}
        found = self.n_both > 0
        for i, q in enumerate(self.QUANTITIES):
            sa, sq, mx, nw, sd = (stats[:, 3 + 5 * i + j].copy() for j in range(5))
            self.sum_abs[q], self.sum_sq[q], self.max_abs[q], self.n_within[q], self.sum_d[q] = sa, sq, mx, nw, sd
            self.errors[q] = dict(mae=nan_ratio(sa, self.n_both) * self.row_spacing,
                                  rmse=np.sqrt(nan_ratio(sq, self.n_both)) * self.row_spacing,
                                  bias=nan_ratio(sd, self.n_both) * self.row_spacing,
                                  max=np.where(found, mx * self.row_spacing, np.nan), within=nan_ratio(nw, self.n_both))

    @classmethod
    def _q(cls, q):
        q = "thickness" if q == "count" else q
        if q not in cls.QUANTITIES:
            raise ValueError(f"quantity must be one of {cls.QUANTITIES} (got {q!r})")
        return q

    def mae(self, k, q="top"):
        """Mean absolute error of class k's top, bottom or thickness, in ``unit``; NaN when no column has the class in both maps."""
        return float(self.errors[self._q(q)]["mae"][k])

    def mean_mae(self, q="top"):
        """The unweighted mean of the classes' MAE over the classes with n_both > 0; NaN when there is none."""
        v = self.errors[self._q(q)]["mae"][self.n_both > 0]
        return float(v.mean()) if v.size else float("nan")

    def to_dict(self):
        lst = lambda a: [float(v) for v in a]
        ints = lambda a: [int(v) for v in a]
        d = dict(K=self.K, rows=self.rows, cols=self.cols, min_run=self.min_run, tol=self.tol, row_spacing=self.row_spacing,
                 unit=self.unit, n_both=ints(self.n_both), n_missing=ints(self.n_missing), n_spurious=ints(self.n_spurious),
                 presence_precision=lst(self.presence_precision), presence_recall=lst(self.presence_recall))
        for q in self.QUANTITIES:
            e = self.errors[q]
            d[q] = dict(mae=lst(e["mae"]), rmse=lst(e["rmse"]), bias=lst(e["bias"]), max=lst(e["max"]),
                        within_tol=lst(e["within"]), sum_abs_rows=ints(self.sum_abs[q]), sum_sq_rows=ints(self.sum_sq[q]),
                        max_abs_rows=ints(self.max_abs[q]), n_within=ints(self.n_within[q]), sum_rows=ints(self.sum_d[q]),
                        mean_mae=self.mean_mae(q))
        if self.dropped is not None:
            d["dropped"] = dict(masked=self.dropped[0], invalid=self.dropped[1])
        return d

    def __str__(self, digits=2):
        num = lambda v, w=9: "{:>{w}}".format("-", w=w) if v != v else "{:>{w}.{d}f}".format(v, w=w, d=digits)
        text = "Horizons (min_run {}, tol {} rows, distances in {}):\n".format(self.min_run, self.tol, self.unit)
        text += "{:>5} {:>9} {:>8} {:>8} {:>8} {:>9} {:>9}  {:>9} {:>9} {:>9} {:>9} {:>9}\n\n".format(
            "class", "quantity", "both", "missing", "spurious", "precision", "recall", "mae", "rmse", "bias", "max", "within")
        for k in range(self.K):
            for i, q in enumerate(self.QUANTITIES):
                lead = "{:>5} {:>9} {:>8} {:>8} {:>8} {} {}".format(
                    k, q, int(self.n_both[k]), int(self.n_missing[k]), int(self.n_spurious[k]), num(self.presence_precision[k]),
                    num(self.presence_recall[k])) if i == 0 else "{:>5} {:>9} {:>8} {:>8} {:>8} {:>9} {:>9}".format("", q, "", "", "", "", "")
                text += lead + "  " + " ".join(num(self.errors[q][x][k]) for x in ("mae", "rmse", "bias", "max", "within")) + "\n"
        text += "\n{:>5} {:>9} {:>8} {:>8} {:>8} {:>9} {:>9}  {}\n".format("mean", "mae", "", "", "", "", "", " ".join(
            "{}={}".format(q, num(self.mean_mae(q), 0).strip()) for q in self.QUANTITIES))
        return text


class Reach:
    """How far do the labels travel?  Accuracy against the distance, in frames, from the nearest labelled trace: one confusion
    matrix per group of columns, from the [groups, K, K] counts, the [groups] confidence sums (None without a confidence map) and
    the dropped quadruple of ``crw_hip.confusion_grouped`` under the column groups of ``crw_hip.column_groups`` (``edges``: its
    edges; group 0 is the labelled columns themselves, group len(edges) + 1 the columns no labelled column reaches).

    ``last_frame`` [groups]: the largest frame distance among each group's columns (-1: the group has no column), so that a
    group the map only partly fills is reported up to the distance it holds.  Per group g: frames[g] = (first, last) frame distance
    (None for the unreached group), pixels / correct [groups] int64, accuracy / mean_iou / mean_confidence [groups] float64 -- NaN
    for an empty group, mean_iou over the classes present in the group, mean_confidence NaN throughout without confidences.
    dropped = (masked, invalid label, invalid confidence, excluded column) or None."""

    def __init__(self, counts, conf_sum=None, dropped=None, edges=crw_hip.REACH_EDGES, last_frame=None):
        host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        counts = np.asarray(host(counts), dtype=np.int64)
        self.edges = [int(e) for e in edges]
        if counts.ndim != 3 or counts.shape[1] != counts.shape[2] or counts.shape[0] != len(self.edges) + 2:
            raise ValueError(f"counts must be [len(edges) + 2, K, K] (got shape {counts.shape} for {len(self.edges)} edges)")
        if (counts < 0).any():
            raise ValueError("counts must be non-negative")
        self.counts, self.groups, self.K = counts, counts.shape[0], counts.shape[1]
        self.unreached = self.groups - 1
        self.dropped = None if dropped is None else tuple(int(v) for v in host(dropped))
        self.conf_sum = None if conf_sum is None else np.asarray(host(conf_sum), dtype=np.float64).reshape(-1)
        if self.conf_sum is not None and self.conf_sum.shape[0] != self.groups:
            raise ValueError(f"conf_sum must hold one sum per group (got {self.conf_sum.shape[0]} for {self.groups} groups)")
        first = [0] + self.edges
        nominal = [e - 1 for e in self.edges] + [None]
        held = [None] * self.groups if last_frame is None else [int(v) for v in host(last_frame)]
        if len(held) != self.groups:
            raise ValueError(f"last_frame must hold one distance per group (got {len(held)} for {self.groups} groups)")
        self.frames = []
        for g in range(self.groups - 1):
            last = nominal[g] if held[g] is None or held[g] < 0 else held[g]
            if last is not None and not first[g] <= last <= (last if nominal[g] is None else nominal[g]):
                raise ValueError(f"group {g} holds frame distances {first[g]} ... {nominal[g]} (last_frame says {last})")
            self.frames.append((first[g], last))
        self.frames.append(None)
        self.pixels = counts.sum((1, 2))
        self.correct = np.trace(counts, axis1=1, axis2=2)
        filled = self.pixels > 0
        nan = np.full(self.groups, np.nan)
        self.accuracy, self.mean_confidence = nan.copy(), nan.copy()
        np.divide(self.correct, self.pixels, out=self.accuracy, where=filled)
        if self.conf_sum is not None:
            np.divide(self.conf_sum, self.pixels, out=self.mean_confidence, where=filled)
        self.mean_iou = np.array([Report(counts[g]).mean_iou if filled[g] else np.nan for g in range(self.groups)])
        self.total = int(self.pixels.sum())

    def report(self, g):
        """``metrics.Report`` of group g: the per-class scores of its pixels."""
        return Report(self.counts[g], None if self.dropped is None else self.dropped[:2])

    def reach_at(self, accuracy):
        """The last frame distance of the longest unbroken run of groups, from group {1} on, that each have at least ``accuracy``;
        empty groups are skipped, the unreached group is never counted, and the result is 0 when the first filled group fails."""
        reach = 0
        for g in range(1, self.unreached):
            if not self.pixels[g]:
                continue
            if not self.accuracy[g] >= accuracy:
                break
            reach = self.frames[g][1] if self.frames[g][1] is not None else self.frames[g][0]
        return int(reach)

    def _name(self, g):
        if g == self.unreached:
            return "unreached"
        a, b = self.frames[g]
        return "{}-".format(a) if b is None else str(a) if a == b else "{}-{}".format(a, b)

    def to_dict(self):
        lst = lambda a: [float(v) for v in a]
        ints = lambda a: [int(v) for v in a]
        d = dict(groups=self.groups, K=self.K, edges=list(self.edges), frames=[None if f is None else list(f) for f in self.frames],
                 pixels=ints(self.pixels), correct=ints(self.correct), accuracy=lst(self.accuracy), mean_iou=lst(self.mean_iou),
                 mean_confidence=lst(self.mean_confidence), total=self.total)
        if self.dropped is not None:
            d["dropped"] = dict(masked=self.dropped[0], invalid=self.dropped[1], invalid_confidence=self.dropped[2],
                                excluded=self.dropped[3])
        return d

    def __str__(self, digits=4):
        num = lambda v: "{:>10}".format("-") if v != v else "{:>10.{d}f}".format(v, d=digits)
        text = "{:>13} {:>12} {:>12} {:>10} {:>10} {:>10}\n\n".format("frames", "pixels", "correct", "accuracy", "mean IoU", "mean conf")
        for g in range(self.groups):
            text += "{:>13} {:>12} {:>12} {} {} {}\n".format(self._name(g), int(self.pixels[g]), int(self.correct[g]), num(self.accuracy[g]),
                                                            num(self.mean_iou[g]), num(self.mean_confidence[g]))
        return text


class HorizonBars:
    """Error bars of the ordered decode's horizon picks against a reference (``inference.horizon_bars``), per boundary k = 1 ...
    S-1 over the ``n`` columns in which the reference has the boundary: ``mae`` of the pick, ``mean_bar`` (the mean error bar,
    sqrt(E[(B_k - pick)^2]) under the decode's posterior) and ``coverage``, the share of those columns whose reference boundary lies
    within z * bar + slack rows of the pick; all in rows, NaN where n = 0.  Built from the four per-boundary sums."""

    def __init__(self, n, sum_abs, sum_bar, n_inside, rows, z=2.0, slack=1.0):
        self.n = np.asarray(n, dtype=np.float64).round().astype(np.int64).reshape(-1)
        self.n_inside = np.asarray(n_inside, dtype=np.float64).round().astype(np.int64).reshape(-1)
        if self.n.shape != self.n_inside.shape or (self.n < 0).any() or (self.n_inside < 0).any() or (self.n_inside > self.n).any():
            raise ValueError("n and n_inside must be one count per boundary with 0 <= n_inside <= n")
        ratio = lambda num: np.divide(np.asarray(num, dtype=np.float64).reshape(-1), self.n, out=np.full(self.n.shape, np.nan),
                                      where=self.n > 0)
        self.mae, self.mean_bar, self.coverage = ratio(sum_abs), ratio(sum_bar), ratio(self.n_inside)
        self.rows, self.z, self.slack = int(rows), float(z), float(slack)

    @property
    def mean_coverage(self):
        """The unweighted mean of the boundaries' coverage over the boundaries the reference has; NaN when there is none."""
        v = self.coverage[self.n > 0]
        return float(v.mean()) if v.size else float("nan")

    def to_dict(self):
        lst = lambda a: [float(v) for v in a]
        return dict(rows=self.rows, z=self.z, slack=self.slack, n=[int(v) for v in self.n], n_inside=[int(v) for v in self.n_inside],
                    mae=lst(self.mae), mean_bar=lst(self.mean_bar), coverage=lst(self.coverage), mean_coverage=self.mean_coverage)

    def __str__(self, digits=2):
        num = lambda v, d=digits: "{:>10}".format("-") if v != v else "{:>10.{d}f}".format(v, d=d)
        text = "Horizon error bars (inside: |reference - pick| <= {:g} x bar + {:g} rows):\n".format(self.z, self.slack)
        text += "{:>8} {:>9} {:>10} {:>10} {:>10}\n\n".format("boundary", "columns", "mae", "mean bar", "inside")
        for k in range(self.n.shape[0]):
            text += "{:>8} {:>9} {} {} {}\n".format(k + 1, int(self.n[k]), num(self.mae[k]), num(self.mean_bar[k]), num(self.coverage[k], 3))
        return text + "\n{:>8} {:>9} {:>10} {:>10} {}\n".format("mean", "", "", "", num(self.mean_coverage, 3))


def _infer_K(gt, pred):
    top = max(float(torch.as_tensor(gt).max()), float(torch.as_tensor(pred).max())) if torch.as_tensor(gt).numel() else 1.0
    if not top == top or top >= 16:
        raise ValueError(f"labels must be integers in [0, 16) (largest: {top})")
    return min(max(int(top) + 1, 2), 16)


def _tensors(gt, pred):
    gt, pred = torch.as_tensor(gt), torch.as_tensor(pred)
    if gt.device != pred.device:  # the reference's call shape: a CPU ground truth against `pred.cpu()` or a device map
        gt = gt.to(pred.device)
    return gt, pred


def classification_report(gt, pred, output_dict=False, digits=2, K=None):
    """``sklearn.metrics.classification_report(gt, pred)``: the text (or, with ``output_dict``, the dict) of a ``Report``."""
    rep = Report.from_maps(*_tensors(gt, pred), K=K)
    if output_dict:
        d = rep.as_dict()
        d.pop("mean_iou")
        for v in d.values():
            if isinstance(v, dict):
                v.pop("iou", None)
        return d
    return rep.__str__(digits)


def confusion_matrix(gt, pred, K=None):
    """``sklearn.metrics.confusion_matrix(gt, pred)``: [n, n] int64 numpy array over the classes present in either map."""
    return Report.from_maps(*_tensors(gt, pred), K=K).matrix
