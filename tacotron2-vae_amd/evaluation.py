"""Summary statistics of `Synthesizer.evaluate` records (pure Python: no torch, no device).

A record is one filelist row scored by free-running synthesis: `dtw` (mel-spectral distortion with dynamic time warping
against the ground-truth mel), `n_frames` (decoded), `n_ref_frames` (ground truth), `hit_max` (decoding ended at
max_decoder_steps instead of at the gate) and `emotion` (label id of the filelist)."""

EMOTIONS = ('neu', 'sad', 'ang', 'hap')      # label ids 0..3 of the koemo filelists (synthesizer.EMOTIONS)


def _median(values):
    v = sorted(values)
    n = len(v)
    return None if n == 0 else v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


def _mean(values):
    return sum(values) / len(values) if values else None


def _stats(records):
    """`dtw_mean` / `dtw_median` cover only the `n_scored` rows whose decoding stopped at the gate: a row that ran to
    max_decoder_steps has no end to align, and its distance says nothing about the model but that it did not stop.  Those
    rows are not hidden: `n_hit_max` and `hit_max_share` count them, and `length_ratio_mean` is over all `n_rows`."""
    stopped = [float(r['dtw']) for r in records if not r['hit_max']]
    n_hit = sum(1 for r in records if r['hit_max'])
    return {'n_rows': len(records),
            'n_hit_max': n_hit,
            'hit_max_share': n_hit / len(records) if records else None,
            'n_scored': len(stopped),
            'dtw_mean': _mean(stopped),
            'dtw_median': _median(stopped),
            'length_ratio_mean': _mean([r['n_frames'] / r['n_ref_frames'] for r in records])}


def summarize(records, emotions=EMOTIONS):
    """{'overall': stats, 'by_emotion': {name: stats}} of evaluate() records; every name of `emotions` appears, with
    n_rows = 0 and None statistics when it has no rows.  A label outside `emotions` is an error."""
    records = list(records)
    for r in records:
        if not 0 <= int(r['emotion']) < len(emotions):
            raise ValueError("emotion label %r outside 0..%d" % (r['emotion'], len(emotions) - 1))
    return {'overall': _stats(records),
            'by_emotion': {name: _stats([r for r in records if int(r['emotion']) == i]) for i, name in enumerate(emotions)}}
