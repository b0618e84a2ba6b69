"""Numbers for the latent space (numpy in fp64: no torch, no device): does the 32-dimensional VAE latent still carry the
speaking style?  `t2v_hip.latent_neighbours` (csrc/latent.hip) does the all-pairs work on the device; the functions here turn
its tensors into scores that can be compared between checkpoints, precisions and KL-annealing schedules.

    knn_predict     the vote of the k nearest labelled neighbours
    silhouette      scikit-learn's silhouette_samples from per-class distance sums and counts
    confusion       counts[true][predicted]
    active_units    latent dimensions whose posterior mean moves over the corpus (Burda et al. 2016, Importance Weighted
                    Autoencoders, section 5.2: Var_x(E[z|x]) > 0.01)
    kl_per_dim      the corpus mean of KL(q(z|x) || N(0, 1)) per latent dimension; a collapsed dimension shows 0
    report          all of them in one JSON-serialisable dict, overall and per emotion
"""
import numpy as np

from evaluation import EMOTIONS

ACTIVE_THRESHOLD = 0.01


def knn_predict(idx, labels, n_classes):
    """(M,) int64 class of each row of idx (M, k), indices into labels, nearest first: the class most of the k neighbours have;
    a tie in votes goes to the class of the nearest neighbour among the tied classes"""
    idx = np.asarray(idx, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    if idx.ndim != 2 or idx.shape[1] < 1:
        raise ValueError("knn_predict: idx must be (M, k) with k >= 1, got %s" % (idx.shape,))
    if labels.size and (labels.min() < 0 or labels.max() >= n_classes):
        raise ValueError("knn_predict: a label outside 0..%d" % (n_classes - 1))
    lab = labels[idx]                                                    # (M, k)
    votes = (lab[:, :, None] == np.arange(n_classes)[None, None, :]).sum(axis=1)          # (M, C)
    tied = votes == votes.max(axis=1, keepdims=True)
    in_tie = np.take_along_axis(tied, lab, 1)                            # (M, k): this neighbour's class is among the tied
    return np.take_along_axis(lab, in_tie.argmax(axis=1)[:, None], 1)[:, 0]


def silhouette(class_sum, class_cnt, own):
    """(M,) fp64 silhouette of each query from class_sum (M, C), the summed distances to the references of each class,
    class_cnt (M, C), their counts, and own (M,), the query's class: a = own sum / own count, b = the smallest mean over the
    other non-empty classes, s = (b - a) / max(a, b).  With the query itself excluded from sums and counts this is
    scikit-learn's silhouette_samples.  s is 0 when the own class has no other member (and when a = b = 0), NaN when no other
    class has a member."""
    class_sum = np.asarray(class_sum, dtype=np.float64)
    class_cnt = np.asarray(class_cnt, dtype=np.int64)
    own = np.asarray(own, dtype=np.int64)
    if class_sum.ndim != 2 or class_sum.shape != class_cnt.shape or own.shape != (len(class_sum),):
        raise ValueError("silhouette: class_sum %s, class_cnt %s, own %s" % (class_sum.shape, class_cnt.shape, own.shape))
    m, c = class_sum.shape
    if m and (own.min() < 0 or own.max() >= c):
        raise ValueError("silhouette: an own class outside 0..%d" % (c - 1))
    rows = np.arange(m)
    is_own = np.arange(c)[None, :] == own[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = class_sum / class_cnt
    other = np.where(is_own | (class_cnt == 0), np.inf, mean)
    b = other.min(axis=1) if c else np.full(m, np.inf)
    n_own = class_cnt[rows, own]
    a = np.where(n_own > 0, class_sum[rows, own] / np.maximum(n_own, 1), 0.0)
    top = np.maximum(a, b)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(top > 0, (b - a) / top, 0.0)
    s = np.where(n_own == 0, 0.0, s)
    return np.where(np.isinf(b), np.nan, s)


def confusion(true, pred, n_classes):
    """(C, C) int64 counts[t][p] of rows with label t predicted as p"""
    true, pred = np.asarray(true, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    if true.shape != pred.shape or true.ndim != 1:
        raise ValueError("confusion: true %s and pred %s must be equal 1-D shapes" % (true.shape, pred.shape))
    for name, v in (('true', true), ('pred', pred)):
        if v.size and (v.min() < 0 or v.max() >= n_classes):
            raise ValueError("confusion: a %s label outside 0..%d" % (name, n_classes - 1))
    out = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(out, (true, pred), 1)
    return out


def active_units(mus, threshold=ACTIVE_THRESHOLD):
    """the number of latent dimensions whose variance of mu over the corpus exceeds the threshold (Burda et al.)"""
    mus = np.asarray(mus, dtype=np.float64)
    if mus.ndim != 2 or len(mus) < 1:
        raise ValueError("active_units: mus must be (N, dims), got %s" % (mus.shape,))
    return int((mus.var(axis=0) > threshold).sum())


def kl_per_dim(mus, logvars):
    """(dims,) fp64: the corpus mean of 1/2 (mu^2 + exp(logvar) - logvar - 1) per dimension"""
    mus, logvars = np.asarray(mus, dtype=np.float64), np.asarray(logvars, dtype=np.float64)
    if mus.ndim != 2 or mus.shape != logvars.shape or len(mus) < 1:
        raise ValueError("kl_per_dim: mus %s and logvars %s must be equal (N, dims) shapes" % (mus.shape, logvars.shape))
    return (0.5 * (mus * mus + np.exp(logvars) - logvars - 1.0)).mean(axis=0)


def _nanmean(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    return float(v.mean()) if len(v) else None


def report(idx, class_sum, class_cnt, labels, mus=None, logvars=None, emotions=EMOTIONS):
    """One JSON-serialisable dict from a leave-one-out `latent_neighbours` call on a labelled corpus: idx (N, k), class_sum and
    class_cnt (N, C) with C = len(emotions), labels (N,).  Holds n, k, knn_accuracy, silhouette_mean (over the rows that have
    one), confusion (rows: true, columns: predicted), by_emotion {name: n, knn_accuracy, silhouette_mean} with None for an
    emotion without rows, and, with mus and logvars, active_units, kl_per_dim and kl_total (their sum)."""
    labels = np.asarray(labels, dtype=np.int64)
    c = len(emotions)
    idx = np.asarray(idx)
    if len(idx) != len(labels):
        raise ValueError("report: %d neighbour rows for %d labels" % (len(idx), len(labels)))
    pred = knn_predict(idx, labels, c)
    sil = silhouette(class_sum, class_cnt, labels)
    hit = pred == labels
    out = {'n': int(len(labels)), 'k': int(idx.shape[1]),
           'knn_accuracy': float(hit.mean()) if len(labels) else None,
           'silhouette_mean': _nanmean(sil),
           'confusion': confusion(labels, pred, c).tolist(),
           'by_emotion': {}}
    for i, name in enumerate(emotions):
        sel = labels == i
        out['by_emotion'][name] = {'n': int(sel.sum()),
                                   'knn_accuracy': float(hit[sel].mean()) if sel.any() else None,
                                   'silhouette_mean': _nanmean(sil[sel]) if sel.any() else None}
    if mus is not None and logvars is not None:
        kl = kl_per_dim(mus, logvars)
        out.update(active_units=active_units(mus), kl_per_dim=[float(v) for v in kl], kl_total=float(kl.sum()))
    return out


def summary_lines(rep):
    """the four lines latent_report.py prints"""
    by = rep['by_emotion']
    fmt = lambda v: 'n/a' if v is None else '%.4f' % v
    lines = ["%d utterances, k = %d: leave-one-out kNN accuracy %s, mean silhouette %s"
             % (rep['n'], rep['k'], fmt(rep['knn_accuracy']), fmt(rep['silhouette_mean'])),
             "kNN accuracy by emotion: " + ", ".join("%s %s" % (n, fmt(by[n]['knn_accuracy'])) for n in by),
             "silhouette by emotion: " + ", ".join("%s %s" % (n, fmt(by[n]['silhouette_mean'])) for n in by)]
    if 'active_units' in rep:
        lines.append("active units %d of %d, KL %.4f nats per utterance" % (rep['active_units'], len(rep['kl_per_dim']),
                                                                           rep['kl_total']))
    else:
        lines.append("active units and KL: not computed (no mus / logvars)")
    return lines


def corpus_report(values, labels, mus=None, logvars=None, k=5, emotions=EMOTIONS):
    """`report` of a labelled corpus of latents: values (N, D) numpy array -> one leave-one-out `t2v_hip.latent_neighbours`
    call on the device.  k is lowered to N - 1 when the corpus is smaller than that."""
    import torch
    import t2v_hip
    values = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
    labels = np.asarray(labels, dtype=np.int64)
    if values.ndim != 2 or len(values) != len(labels):
        raise ValueError("corpus_report: values %s for %d labels" % (values.shape, len(labels)))
    if len(values) < 2:
        raise ValueError("corpus_report: %d utterances; at least 2 are needed" % len(values))
    k = min(int(k), len(values) - 1)
    r = t2v_hip.latent_neighbours(torch.from_numpy(values).cuda(), labels, k=k, n_classes=len(emotions))
    return report(r.idx.cpu().numpy(), r.class_sum.cpu().numpy(), r.class_cnt.cpu().numpy(), labels, mus, logvars, emotions)
