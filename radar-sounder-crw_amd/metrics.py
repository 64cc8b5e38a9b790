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
