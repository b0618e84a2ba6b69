"""Summary statistics of `Synthesizer.evaluate` records (pure Python: no torch, no device).

A record is one filelist row scored by free-running synthesis: `dtw` (mel-spectral distortion with dynamic time warping
against the ground-truth mel), `n_frames` (decoded), `n_ref_frames` (ground truth), `hit_max` (decoding ended at
max_decoder_steps instead of at the gate) and `emotion` (label id of the filelist).

`evaluate(prosody=True)` adds the pitch of both sides (`t2v_hip.f0` on the Griffin-Lim waveform of the synthesised mel and
on the recording): `f0_median_hz` / `f0_ref_median_hz` (median over voiced frames), `f0_spread_st` / `f0_ref_spread_st`
(standard deviation of 12 log2(f0 / median) over voiced frames, in semitones), `voiced_share` / `voiced_ref_share` and
`f0_shift_st` = 12 log2(f0_median_hz / f0_ref_median_hz).  The F0 values of a side with fewer than MIN_VOICED_FRAMES voiced
frames are None, and so is the shift when either side's are.

`evaluate(alignment=True)` adds what the attention alignment says about reading the text (`t2v_hip.alignment_stats` on the
decoder's alignments; p[t] is the text position frame t attends most, L = `n_symbols`): `focus` (mean weight on p[t]), `reach`
((furthest p + 1) / L), `end_reach` ((p of the last frame + 1) / L), `back_share` and `jump_share` (steps back, and steps
forward by more than max_jump, over the n_frames - 1 transitions), `stall_frames` (longest run of frames on one position),
`uncovered_share` (positions whose summed weight stays under cover_min, over L) and `gap_symbols` (longest run of such
positions).  `summarize` cuts them into `read_through_share` with END_SLACK, GAP_MIN and BACK_SLACK.  Those three and the
kernel's max_jump = 3 and cover_min = 0.5 are choices, not measurements (no trained checkpoint exists here); the raw per-row
numbers are always in the records, so they can be cut again.

`evaluate(style=True)` adds the style round trip (`t2v_hip.latent_neighbours` on the posterior means): the synthesised mel
is encoded again, and its mu is placed among the mu of the distinct recordings of the filelist, its own recording left out of
the vote.  `style_emotion` is the vote of the k nearest other recordings, `style_hit` whether that is the row's label,
`style_own_rank` how many recordings lie closer than the row's own (0: the synthesis is nearest to the clip it copied),
`style_own_dist` the distance to it, and `style_silhouette` the silhouette of the synthesised mu against the recorded clusters
with the row's label as its own class.  All five are None for a row decoded to fewer frames than the encoder takes (and the
silhouette alone where it is undefined).  `summarize` adds a `style` block, whose `ref_accuracy`, the leave-one-out accuracy
of the recordings themselves under the same k, is the ceiling the synthesised accuracy has to be read against.

`evaluate(aligned=True)` adds the frame-aligned numbers of the prosody-transfer papers (`t2v_hip.aligned_scores`): a DTW over
13 mel-cepstral coefficients of both mels gives the warping path, and along its K points `mcd_db` (MCD-13, from the 80-band
log-mel: (10 / ln 10) sqrt(2) times the mean cepstral distance), `warp_dev` (mean |i / (Tx - 1) - j / (Ty - 1)|: how far the
synthesis is stretched unevenly against the recording, 0 for a linear stretch) and, when the pitch tracks are there
(prosody=True), `vde` (voicing decision error: one side voiced, over K), `gpe` (gross pitch error: more than 20 % apart, over
the both-voiced points), `ffe` (either, over K), `lf0_rmse_cents`, `lf0_bias_cents` and `lf0_corr` (Pearson, of log F0 over
the both-voiced points).  The F0 values are None without tracks; gpe and the three log-F0 values also when no point is voiced
on both sides, and the correlation under 2 such points or at a zero variance.

`evaluate(energy=True)` adds the third correlate of prosody, the level (`t2v_hip.loudness`, the K-weighted gated loudness of
ITU-R BS.1770-4, on the Griffin-Lim waveform of the synthesised mel and on the recording): `loudness_lufs` /
`loudness_ref_lufs`, `loudness_shift_lu` = synthesis - recording, and `energy_spread_db` / `energy_ref_spread_db`, the standard
deviation of the K-weighted frame level in dB over the sounding frames, those within ENERGY_FLOOR_DB of the row's loudest
frame (the trim's rule; like the alignment thresholds an uncalibrated choice, not a measurement).  A side without a loudness
(no waveform, shorter than one 400 ms block, or below the gates) has None.  With aligned=True as well, `energy_rmse_db` and
`energy_corr` (Pearson) compare the two dB tracks along the warping path, over the points where both sides sound.  `summarize`
adds an `energy` block.

`evaluate(voice=True)` adds the fourth correlate, voice quality (`t2v_hip.voice_quality` on the same two waveforms): the
spectral-balance descriptors of eGeMAPS and the cepstral peak prominence, each the median over the side's counted frames (not
silent and within VOICE_FLOOR_DB of the row's loudest frame): `alpha_db` / `alpha_ref_db` (1 - 5 kHz over 50 Hz - 1 kHz; a
pressed voice has more), `hammarberg_db` / `hammarberg_ref_db` (the peak below 2 kHz over the peak in 2 - 5 kHz), `slope_db_khz`
/ `slope_ref_db_khz` (over 500 - 1500 Hz), `cpp_db` / `cpp_ref_db` (a breathy voice has a weak cepstral peak), and
`alpha_shift_db` and `cpp_shift_db` = synthesis - recording.  A side without a counted frame or without a waveform has None.
With aligned=True as well, `alpha_rmse_db` and `alpha_corr` compare the two alpha_db tracks along the warping path, over the
points where both frames are counted.  `summarize` adds a `voice` block.

`evaluate(durations=True)` adds the timing per symbol (`t2v_hip.mas`, the best monotonic path through an alignment matrix): the
free-running alignments of the synthesis and the teacher-forced alignments of the recording are each forced onto the row's
text, which gives frames per symbol on both sides.  `dur_rmse_frames`, `dur_corr` (Pearson over the symbols) and
`dur_log_ratio_spread` (standard deviation of ln((1 + d_syn) / (1 + d_rec)): 0 for a uniform change of tempo) compare them;
`align_logp_syn` / `align_logp_rec` are the mean log attention weight along each path (low: the text does not match).  With
prosody=True as well, `seg_f0_rmse_cents` and `seg_f0_corr` compare the mean F0 per symbol (`t2v_hip.segment_means` over the
voiced frames) on the symbols voiced on both sides.  A side without a feasible path (more symbols than frames can reach) has
None.  `summarize` adds `n_durations` and the means to every stats dict."""
import math

EMOTIONS = ('neu', 'sad', 'ang', 'hap')      # label ids 0..3 of the koemo filelists (synthesizer.EMOTIONS)


def _median(values):
    v = sorted(values)
    n = len(v)
    return None if n == 0 else v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])


def _mean(values):
    return sum(values) / len(values) if values else None


MIN_VOICED_FRAMES = 5
PROSODY_KEYS = ('f0_median_hz', 'f0_ref_median_hz', 'f0_spread_st', 'f0_ref_spread_st', 'voiced_share', 'voiced_ref_share',
                'f0_shift_st')


def pitch_stats(track):
    """(median Hz, spread in semitones, voiced share) of one F0 track (Hz per frame, 0 where unvoiced): the spread is the
    standard deviation of 12 log2(f0 / median) over the voiced frames; median and spread are None under MIN_VOICED_FRAMES
    voiced frames, the share is None for an empty track."""
    track = [float(v) for v in track]
    voiced = [v for v in track if v > 0.0]
    share = len(voiced) / len(track) if track else None
    if len(voiced) < MIN_VOICED_FRAMES:
        return None, None, share
    med = _median(voiced)
    st = [12.0 * math.log2(v / med) for v in voiced]
    mean = sum(st) / len(st)
    return med, math.sqrt(sum((v - mean) ** 2 for v in st) / len(st)), share


def prosody_fields(track, ref_track):
    """the PROSODY_KEYS of one record from the F0 tracks of the synthesised waveform and of the recording (track: None when
    the row has no waveform, i.e. fewer than the vocoder's 4 frames)"""
    med, spread, share = pitch_stats(track) if track is not None else (None, None, None)
    rmed, rspread, rshare = pitch_stats(ref_track)
    return {'f0_median_hz': med, 'f0_ref_median_hz': rmed, 'f0_spread_st': spread, 'f0_ref_spread_st': rspread,
            'voiced_share': share, 'voiced_ref_share': rshare,
            'f0_shift_st': 12.0 * math.log2(med / rmed) if med is not None and rmed is not None else None}


def _prosody_stats(records):
    """Over the rows that stopped at the gate (a row that ran to max_decoder_steps has no end, and its waveform's tail says
    nothing about the style): `n_prosody` of them have a pitch on both sides (`f0_shift_st` not None) and carry
    `f0_shift_st_mean` (signed: a bias), `f0_shift_st_abs_mean` and `f0_spread_ratio_mean` (synthesised spread / recording's
    spread, over the rows whose recording's spread is not 0; far below 1 is the flat-voice failure).  The voiced shares are
    means over every stopped row that has one, so a model whose output is never voiced shows here and in n_prosody."""
    stopped = [r for r in records if not r['hit_max']]
    rows = [r for r in stopped if r.get('f0_shift_st') is not None]
    return {'n_prosody': len(rows),
            'f0_shift_st_mean': _mean([r['f0_shift_st'] for r in rows]),
            'f0_shift_st_abs_mean': _mean([abs(r['f0_shift_st']) for r in rows]),
            'f0_spread_ratio_mean': _mean([r['f0_spread_st'] / r['f0_ref_spread_st'] for r in rows if r['f0_ref_spread_st'] > 0]),
            'voiced_share_mean': _mean([r['voiced_share'] for r in stopped if r.get('voiced_share') is not None]),
            'voiced_ref_share_mean': _mean([r['voiced_ref_share'] for r in stopped if r.get('voiced_ref_share') is not None])}


ALIGNMENT_KEYS = ('focus', 'reach', 'end_reach', 'back_share', 'jump_share', 'stall_frames', 'uncovered_share', 'gap_symbols',
                  'n_symbols')
END_SLACK = 3        # read through: the last frame attends one of the last END_SLACK + 1 text positions,
GAP_MIN = 4          # no GAP_MIN consecutive positions stay uncovered,
BACK_SLACK = 2       # and at most BACK_SLACK transitions go back.  Uncalibrated choices (module docstring).


def alignment_fields(focus, stats_row, n_frames, n_symbols):
    """the ALIGNMENT_KEYS of one record from one row of `t2v_hip.alignment_stats`: focus, the stats columns (furthest, p_last,
    n_back, n_jump, longest_stall, n_uncovered, longest_gap, in t2v_hip.ALIGN_STATS order; a reserved eighth word is ignored),
    the row's frame count and its number of text symbols.  The shares of back-steps and jumps are over the n_frames - 1
    transitions, 0.0 for a single frame."""
    furthest, p_last, n_back, n_jump, stall, n_unc, gap = [int(v) for v in list(stats_row)[:7]]
    n, L = int(n_frames), int(n_symbols)
    if n < 1 or L < 1:
        raise ValueError("alignment_fields: %d frames, %d symbols; both must be >= 1" % (n, L))
    steps = n - 1
    return {'focus': float(focus), 'reach': (furthest + 1) / L, 'end_reach': (p_last + 1) / L,
            'back_share': n_back / steps if steps else 0.0, 'jump_share': n_jump / steps if steps else 0.0,
            'stall_frames': stall, 'uncovered_share': n_unc / L, 'gap_symbols': gap, 'n_symbols': L}


def reads_through(record, end_slack=END_SLACK, gap_min=GAP_MIN, back_slack=BACK_SLACK):
    """the last frame attends a position within end_slack of the text's end, fewer than gap_min consecutive positions stay
    uncovered, and at most back_slack transitions go back"""
    L = record['n_symbols']
    n_back = round(record['back_share'] * (record['n_frames'] - 1))
    return bool(round(record['end_reach'] * L) >= L - end_slack and record['gap_symbols'] < gap_min and n_back <= back_slack)


def _alignment_stats(records, end_slack=END_SLACK, gap_min=GAP_MIN, back_slack=BACK_SLACK):
    """Over the `n_alignment` rows that stopped at the gate (the alignment of a row that ran to max_decoder_steps has no end to
    reach): the means of focus, reach, back_share, jump_share and uncovered_share, mean and max of stall_frames and
    gap_symbols, and `n_read_through` / `read_through_share`, the rows `reads_through` accepts."""
    rows = [r for r in records if not r['hit_max'] and 'n_symbols' in r]
    out = {'n_alignment': len(rows)}
    for k in ('focus', 'reach', 'back_share', 'jump_share', 'uncovered_share'):
        out[k + '_mean'] = _mean([r[k] for r in rows])
    for k in ('stall_frames', 'gap_symbols'):
        out[k + '_mean'] = _mean([r[k] for r in rows])
        out[k + '_max'] = max([r[k] for r in rows]) if rows else None
    n_read = sum(1 for r in rows if reads_through(r, end_slack, gap_min, back_slack))
    out['n_read_through'] = n_read
    out['read_through_share'] = n_read / len(rows) if rows else None
    return out


ALIGNED_KEYS = ('mcd_db', 'vde', 'gpe', 'ffe', 'lf0_rmse_cents', 'lf0_bias_cents', 'lf0_corr', 'warp_dev')
ALIGNED_MEANS = ('mcd_db', 'vde', 'gpe', 'ffe', 'lf0_rmse_cents', 'lf0_corr', 'warp_dev')
MCD_DB = 10.0 / math.log(10.0) * math.sqrt(2.0)


def aligned_fields(counts, sums, f0=True):
    """the ALIGNED_KEYS of one record from one row of `t2v_hip.aligned_scores`: counts (n_points, n_both, n_vde, n_gpe, in
    t2v_hip.ALIGNED_COUNTS order) and sums (sum_d, sum_e, sum_e2, s_xx, s_yy, s_xy, sum_warp, in t2v_hip.ALIGNED_SUMS order; a
    reserved eighth word is ignored), divided here in fp64.  f0=False: the row had no pitch tracks, and its six F0 values are
    None (not 0).  A refused row (n_points 0) has None everywhere."""
    K, n_both, n_vde, n_gpe = [int(v) for v in list(counts)[:4]]
    sum_d, sum_e, sum_e2, s_xx, s_yy, s_xy, sum_warp = [float(v) for v in list(sums)[:7]]
    out = dict.fromkeys(ALIGNED_KEYS)
    if K < 1:
        return out
    out['mcd_db'] = MCD_DB * sum_d / K
    out['warp_dev'] = sum_warp / K
    if not f0:
        return out
    out['vde'] = n_vde / K
    out['ffe'] = (n_vde + n_gpe) / K
    if n_both > 0:
        out['gpe'] = n_gpe / n_both
        out['lf0_rmse_cents'] = math.sqrt(sum_e2 / n_both)
        out['lf0_bias_cents'] = sum_e / n_both
        if n_both >= 2 and s_xx > 0.0 and s_yy > 0.0:
            out['lf0_corr'] = max(-1.0, min(1.0, s_xy / math.sqrt(s_xx * s_yy)))
    return out


def _aligned_stats(records):
    """Over the `n_aligned` rows that stopped at the gate and carry the aligned keys (a row that ran to max_decoder_steps has
    no end to align): the mean of each of ALIGNED_MEANS over the rows that have that value."""
    rows = [r for r in records if not r['hit_max'] and 'mcd_db' in r]
    out = {'n_aligned': len(rows)}
    for k in ALIGNED_MEANS:
        out[k + '_mean'] = _mean([r[k] for r in rows if r.get(k) is not None])
    return out


ENERGY_KEYS = ('loudness_lufs', 'loudness_ref_lufs', 'loudness_shift_lu', 'energy_spread_db', 'energy_ref_spread_db')
ENERGY_ALIGNED_KEYS = ('energy_rmse_db', 'energy_corr')
ENERGY_FLOOR_DB = 40.0   # a frame sounds within this many dB of the row's loudest frame.  An uncalibrated choice (module docstring).


def sounding_frames(track_db, floor_db=ENERGY_FLOOR_DB):
    """one bool per frame of a dB track: within floor_db of the loudest frame"""
    track = [float(v) for v in track_db]
    top = max(track) if track else 0.0
    return [v > top - floor_db for v in track]


def energy_spread(track_db, floor_db=ENERGY_FLOOR_DB):
    """standard deviation of the frame level in dB over the sounding frames; None for an empty track"""
    track = [float(v) for v in track_db]
    v = [x for x, s in zip(track, sounding_frames(track, floor_db)) if s]
    if not v:
        return None
    mean = sum(v) / len(v)
    return math.sqrt(sum((x - mean) ** 2 for x in v) / len(v))


def _finite(v):
    return None if v is None or math.isinf(v) or math.isnan(v) else float(v)


def energy_fields(loudness, track_db, ref_loudness, ref_track_db):
    """the ENERGY_KEYS of one record from the integrated loudness (LUFS) and the frame level track (dB) of the synthesised
    waveform and of the recording.  loudness and track_db are None when the row has no waveform (fewer than the vocoder's 4
    frames); a loudness of -inf (no gated block) becomes None, and so does the shift when either side's is."""
    lu, ref = _finite(loudness), _finite(ref_loudness)
    return {'loudness_lufs': lu, 'loudness_ref_lufs': ref,
            'loudness_shift_lu': lu - ref if lu is not None and ref is not None else None,
            'energy_spread_db': energy_spread(track_db) if track_db is not None else None,
            'energy_ref_spread_db': energy_spread(ref_track_db) if ref_track_db is not None else None}


def _path_rmse_corr(pairs):
    """(root mean square difference, Pearson correlation) of (synthesis, recording) pairs: both None without a pair, the
    correlation also under 2 pairs or at a zero variance"""
    pairs = [(float(a), float(b)) for a, b in pairs]
    if not pairs:
        return None, None
    n = len(pairs)
    rmse = math.sqrt(sum((a - b) ** 2 for a, b in pairs) / n)
    ma, mb = sum(a for a, _ in pairs) / n, sum(b for _, b in pairs) / n
    sxx, syy = sum((a - ma) ** 2 for a, _ in pairs), sum((b - mb) ** 2 for _, b in pairs)
    if n >= 2 and sxx > 0.0 and syy > 0.0:
        return rmse, max(-1.0, min(1.0, sum((a - ma) * (b - mb) for a, b in pairs) / math.sqrt(sxx * syy)))
    return rmse, None


def energy_path_fields(pairs):
    """the ENERGY_ALIGNED_KEYS from the (synthesis dB, recording dB) pairs at the warping path's points where both sides sound:
    the root mean square difference and the Pearson correlation (None under 2 points or at a zero variance)"""
    return dict(zip(ENERGY_ALIGNED_KEYS, _path_rmse_corr(pairs)))


def _energy_stats(records):
    """Over the rows that stopped at the gate: `n_energy` of them have a loudness on both sides and carry
    `loudness_shift_lu_mean` (signed), `loudness_shift_lu_abs_mean` and `energy_spread_ratio_mean` (synthesised spread /
    recording's, over the rows whose recording's spread is not 0; far below 1 is a flat level contour); with the aligned keys
    also `energy_rmse_db_mean` and `energy_corr_mean`, over the rows that have the value."""
    stopped = [r for r in records if not r['hit_max']]
    rows = [r for r in stopped if r.get('loudness_shift_lu') is not None]
    out = {'n_energy': len(rows),
           'loudness_shift_lu_mean': _mean([r['loudness_shift_lu'] for r in rows]),
           'loudness_shift_lu_abs_mean': _mean([abs(r['loudness_shift_lu']) for r in rows]),
           'energy_spread_ratio_mean': _mean([r['energy_spread_db'] / r['energy_ref_spread_db'] for r in rows
                                              if r.get('energy_spread_db') is not None and r.get('energy_ref_spread_db')])}
    if any('energy_rmse_db' in r for r in records):
        for k in ENERGY_ALIGNED_KEYS:
            out[k + '_mean'] = _mean([r[k] for r in stopped if r.get(k) is not None])
    return out


def _energy_block(records, emotions):
    """the `energy` entry of summarize(): overall and by_emotion `_energy_stats`; every emotion also carries
    `loudness_vs_neu_lu` and `loudness_ref_vs_neu_lu`, the mean loudness of its stopped rows minus that of the emotion named
    'neu', for the synthesis and for the recordings (None where either has no row with a loudness, or no 'neu' is listed):
    whether the emotions keep their level order."""
    stopped = [r for r in records if not r['hit_max']]

    def level(i, key):
        return _mean([r[key] for r in stopped if int(r['emotion']) == i and r.get(key) is not None])

    neu = list(emotions).index('neu') if 'neu' in emotions else None
    by = {}
    for i, name in enumerate(emotions):
        st = _energy_stats([r for r in records if int(r['emotion']) == i])
        for key, out_key in (('loudness_lufs', 'loudness_vs_neu_lu'), ('loudness_ref_lufs', 'loudness_ref_vs_neu_lu')):
            a, b = level(i, key), level(neu, key) if neu is not None else None
            st[out_key] = a - b if a is not None and b is not None else None
        by[name] = st
    return {'overall': _energy_stats(records), 'by_emotion': by}


VOICE_KEYS = ('alpha_db', 'alpha_ref_db', 'alpha_shift_db', 'hammarberg_db', 'hammarberg_ref_db', 'slope_db_khz', 'slope_ref_db_khz',
              'cpp_db', 'cpp_ref_db', 'cpp_shift_db')
VOICE_ALIGNED_KEYS = ('alpha_rmse_db', 'alpha_corr')
VOICE_TRACKS = ('level_db', 'alpha_db', 'hammarberg_db', 'slope_db_khz', 'cpp_db')      # the planes voice_fields reads
VOICE_SILENT_DB = -200.0   # level_db of a frame without energy (T2V_VOICE_SILENT_DB)
VOICE_FLOOR_DB = 40.0      # a frame is counted within this many dB of the row's loudest frame: ENERGY_FLOOR_DB's rule


def voice_counted(level_db, floor_db=VOICE_FLOOR_DB):
    """one bool per frame of a level_db track: not silent and within floor_db of the loudest frame that is not; a track of
    silent frames alone has none (`t2v_hip.voice_counted` on the host)"""
    track = [float(v) for v in level_db]
    heard = [v for v in track if v > VOICE_SILENT_DB]
    top = max(heard) if heard else 0.0
    return [v > VOICE_SILENT_DB and v > top - floor_db for v in track]


def voice_medians(tracks):
    """{plane: median over the counted frames} of one side's VOICE_TRACKS (a dict of per-frame lists), the four planes
    behind level_db; None everywhere for a side without a waveform (tracks None) or without a counted frame"""
    names = VOICE_TRACKS[1:]
    if tracks is None:
        return dict.fromkeys(names)
    keep = voice_counted(tracks['level_db'])
    return {k: _median([float(v) for v, c in zip(tracks[k], keep) if c]) for k in names}


def voice_fields(syn_tracks, ref_tracks):
    """the VOICE_KEYS of one record from the voice-quality tracks (`t2v_hip.voice_quality`, cut to the side's frames) of the
    synthesised waveform and of the recording: each value the median over its side's counted frames, the two shifts synthesis
    minus recording.  syn_tracks is None when the row has no waveform (fewer than the vocoder's 4 frames)."""
    syn, ref = voice_medians(syn_tracks), voice_medians(ref_tracks)

    def shift(k):
        return syn[k] - ref[k] if syn[k] is not None and ref[k] is not None else None
    return {'alpha_db': syn['alpha_db'], 'alpha_ref_db': ref['alpha_db'], 'alpha_shift_db': shift('alpha_db'),
            'hammarberg_db': syn['hammarberg_db'], 'hammarberg_ref_db': ref['hammarberg_db'],
            'slope_db_khz': syn['slope_db_khz'], 'slope_ref_db_khz': ref['slope_db_khz'],
            'cpp_db': syn['cpp_db'], 'cpp_ref_db': ref['cpp_db'], 'cpp_shift_db': shift('cpp_db')}


def voice_path_fields(pairs):
    """the VOICE_ALIGNED_KEYS from the (synthesis, recording) alpha_db pairs at the warping path's points where both frames
    are counted, as `energy_path_fields`"""
    return dict(zip(VOICE_ALIGNED_KEYS, _path_rmse_corr(pairs)))


def _voice_stats(records):
    """Over the rows that stopped at the gate: `n_voice` of them have an alpha ratio on both sides (`alpha_shift_db` not
    None); `<key>_mean` for every key of VOICE_KEYS, and with the aligned keys of VOICE_ALIGNED_KEYS, over the rows that have
    the value."""
    stopped = [r for r in records if not r['hit_max']]
    out = {'n_voice': sum(1 for r in stopped if r.get('alpha_shift_db') is not None)}
    keys = VOICE_KEYS + (VOICE_ALIGNED_KEYS if any('alpha_rmse_db' in r for r in records) else ())
    for k in keys:
        out[k + '_mean'] = _mean([r[k] for r in stopped if r.get(k) is not None])
    return out


def _voice_block(records, emotions):
    """the `voice` entry of summarize(): overall and by_emotion `_voice_stats`; every emotion also carries `alpha_vs_neu_db`,
    `alpha_ref_vs_neu_db`, `cpp_vs_neu_db` and `cpp_ref_vs_neu_db`, the mean alpha_db and cpp_db of its stopped rows minus
    those of the emotion named 'neu', for the synthesis and for the recordings (None where either has no row with the value,
    or no 'neu' is listed): whether the emotions keep their order of tilt and of breathiness.  No thresholds."""
    stopped = [r for r in records if not r['hit_max']]

    def level(i, key):
        return _mean([r[key] for r in stopped if int(r['emotion']) == i and r.get(key) is not None])

    neu = list(emotions).index('neu') if 'neu' in emotions else None
    by = {}
    for i, name in enumerate(emotions):
        st = _voice_stats([r for r in records if int(r['emotion']) == i])
        for key, out_key in (('alpha_db', 'alpha_vs_neu_db'), ('alpha_ref_db', 'alpha_ref_vs_neu_db'),
                             ('cpp_db', 'cpp_vs_neu_db'), ('cpp_ref_db', 'cpp_ref_vs_neu_db')):
            a, b = level(i, key), level(neu, key) if neu is not None else None
            st[out_key] = a - b if a is not None and b is not None else None
        by[name] = st
    return {'overall': _voice_stats(records), 'by_emotion': by}


DURATION_KEYS = ('dur_rmse_frames', 'dur_corr', 'dur_log_ratio_spread', 'align_logp_syn', 'align_logp_rec')
DURATION_F0_KEYS = ('seg_f0_rmse_cents', 'seg_f0_corr')


def _pearson(x, y):
    """Pearson correlation of two equally long fp64 lists; None under 2 values or at a zero variance"""
    n = len(x)
    if n < 2:
        return None
    mx, my = sum(x) / n, sum(y) / n
    sxx, syy = sum((a - mx) ** 2 for a in x), sum((b - my) ** 2 for b in y)
    if not (sxx > 0.0 and syy > 0.0):
        return None
    return max(-1.0, min(1.0, sum((a - mx) * (b - my) for a, b in zip(x, y)) / math.sqrt(sxx * syy)))


def duration_fields(d_syn, d_rec, logp_syn, logp_rec):
    """the DURATION_KEYS of one record from the symbol durations (frames per symbol, `t2v_hip.mas`) of the synthesis and of the
    recording over the same symbols, and the two mean log-probabilities along the paths.  A side without a feasible path
    (durations None) leaves the three comparisons None and keeps the other side's align_logp.  dur_rmse_frames: root mean
    square of d_syn - d_rec over the symbols; dur_corr: their Pearson correlation (None under 2 symbols or at a zero variance);
    dur_log_ratio_spread: the standard deviation over the symbols of ln((1 + d_syn) / (1 + d_rec)), 0 when every symbol is
    stretched alike."""
    out = dict.fromkeys(DURATION_KEYS)
    out['align_logp_syn'] = None if logp_syn is None or d_syn is None else _finite(logp_syn)
    out['align_logp_rec'] = None if logp_rec is None or d_rec is None else _finite(logp_rec)
    if d_syn is None or d_rec is None:
        return out
    a, b = [float(v) for v in d_syn], [float(v) for v in d_rec]
    if len(a) != len(b) or not a:
        raise ValueError("duration_fields: %d and %d symbols; both sides are searched over the same text" % (len(a), len(b)))
    L = len(a)
    out['dur_rmse_frames'] = math.sqrt(sum((u - v) ** 2 for u, v in zip(a, b)) / L)
    out['dur_corr'] = _pearson(a, b)
    ratio = [math.log((1.0 + u) / (1.0 + v)) for u, v in zip(a, b)]
    mean = sum(ratio) / L
    out['dur_log_ratio_spread'] = math.sqrt(sum((r - mean) ** 2 for r in ratio) / L)
    return out


def segment_f0_fields(sum_syn, count_syn, sum_rec, count_rec):
    """the DURATION_F0_KEYS of one record from `t2v_hip.segment_means` of both sides' F0 tracks over their voiced frames (sums in
    Hz and counts per symbol; None for a side without a track or a path): the mean F0 of a symbol is sum / count, the symbols
    with a voiced frame on both sides are compared.  seg_f0_rmse_cents: root mean square of 1200 log2(syn / rec); seg_f0_corr:
    Pearson correlation of the two log2 means.  None without such a symbol (the correlation also under 2, or at a zero
    variance)."""
    out = dict.fromkeys(DURATION_F0_KEYS)
    if sum_syn is None or sum_rec is None:
        return out
    pairs = [(math.log2(float(s) / c), math.log2(float(r) / k))
             for s, c, r, k in zip(sum_syn, count_syn, sum_rec, count_rec) if c > 0 and k > 0 and s > 0 and r > 0]
    if not pairs:
        return out
    out['seg_f0_rmse_cents'] = 1200.0 * math.sqrt(sum((u - v) ** 2 for u, v in pairs) / len(pairs))
    out['seg_f0_corr'] = _pearson([u for u, _ in pairs], [v for _, v in pairs])
    return out


def _duration_stats(records):
    """Over the `n_durations` rows that stopped at the gate and have durations on both sides (`dur_rmse_frames` not None; a row
    that ran to max_decoder_steps has no end to force the path to): the mean of each of DURATION_KEYS, and of
    DURATION_F0_KEYS when the records carry them, over the rows that have the value."""
    stopped = [r for r in records if not r['hit_max']]
    out = {'n_durations': sum(1 for r in stopped if r.get('dur_rmse_frames') is not None)}
    keys = DURATION_KEYS + (DURATION_F0_KEYS if any('seg_f0_corr' in r for r in records) else ())
    for k in keys:
        out[k + '_mean'] = _mean([r[k] for r in stopped if r.get(k) is not None])
    return out


STYLE_KEYS = ('style_emotion', 'style_hit', 'style_own_rank', 'style_own_dist', 'style_silhouette')


class StyleRecords(list):
    """the records of evaluate(style=True): a list, plus `style_info` = {'k', 'n_recordings', 'ref_accuracy'}, what the
    recordings say about themselves, for `summarize`"""
    style_info = None


def style_fields(emotion, vote, own_rank, own_dist, silhouette):
    """the STYLE_KEYS of one record; vote None: the row has no style fields (all None)"""
    if vote is None:
        return dict.fromkeys(STYLE_KEYS)
    sil = None if silhouette is None or math.isnan(silhouette) else float(silhouette)
    return {'style_emotion': int(vote), 'style_hit': bool(int(vote) == int(emotion)), 'style_own_rank': int(own_rank),
            'style_own_dist': float(own_dist), 'style_silhouette': sil}


def _style_stats(records):
    """Over the `n_style` rows that have style fields (a row without them is counted out, not as a miss): `accuracy` (share of
    style_hit), `rank0_share` (share whose own recording is the nearest of all), `rank_median` and `silhouette_mean` (over the
    rows that have a silhouette)."""
    rows = [r for r in records if r.get('style_emotion') is not None]
    return {'n_style': len(rows),
            'accuracy': _mean([1.0 if r['style_hit'] else 0.0 for r in rows]),
            'rank0_share': _mean([1.0 if r['style_own_rank'] == 0 else 0.0 for r in rows]),
            'rank_median': _median([r['style_own_rank'] for r in rows]),
            'silhouette_mean': _mean([r['style_silhouette'] for r in rows if r['style_silhouette'] is not None])}


def _style_block(records, emotions, info):
    """the `style` entry of summarize(): overall, by_emotion, the confusion matrix (rows: the label, columns: the vote) and
    what `info` holds (k, n_recordings, ref_accuracy; None where the caller has no info)"""
    info = info or {}
    conf = [[0] * len(emotions) for _ in emotions]
    for r in records:
        if r.get('style_emotion') is not None:
            conf[int(r['emotion'])][int(r['style_emotion'])] += 1
    return {'k': info.get('k'), 'n_recordings': info.get('n_recordings'), 'ref_accuracy': info.get('ref_accuracy'),
            'overall': _style_stats(records),
            'by_emotion': {name: _style_stats([r for r in records if int(r['emotion']) == i]) for i, name in enumerate(emotions)},
            'confusion': conf}


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


def summarize(records, emotions=EMOTIONS, end_slack=END_SLACK, gap_min=GAP_MIN, back_slack=BACK_SLACK, style_info=None):
    """{'overall': stats, 'by_emotion': {name: stats}} of evaluate() records; every name of `emotions` appears, with
    n_rows = 0 and None statistics when it has no rows.  A label outside `emotions` is an error.  When the records carry
    the prosody keys (evaluate(prosody=True)) every stats dict also holds those of `_prosody_stats`; when they carry the
    alignment keys (evaluate(alignment=True)), those of `_alignment_stats`, cut with end_slack, gap_min and back_slack; when
    they carry the aligned keys (evaluate(aligned=True)), `n_aligned` and the means of `_aligned_stats`; when they carry the
    duration keys (evaluate(durations=True)), `n_durations` and the means of `_duration_stats`.
    When they carry the style keys (evaluate(style=True)) the result gains 'style': `_style_block`, with k, n_recordings and
    ref_accuracy from style_info, else from the records' own `style_info` (StyleRecords), else None.
    When they carry the energy keys (evaluate(energy=True)) the result gains 'energy': `_energy_block`; when they carry the
    voice keys (evaluate(voice=True)), 'voice': `_voice_block`."""
    if style_info is None:
        style_info = getattr(records, 'style_info', None)
    records = list(records)
    for r in records:
        if not 0 <= int(r['emotion']) < len(emotions):
            raise ValueError("emotion label %r outside 0..%d" % (r['emotion'], len(emotions) - 1))
    prosody = any('f0_shift_st' in r for r in records)
    alignment = any('n_symbols' in r for r in records)
    aligned = any('mcd_db' in r for r in records)
    durations = any('dur_rmse_frames' in r for r in records)

    def stats(rows):
        out = _stats(rows)
        if prosody:
            out.update(_prosody_stats(rows))
        if alignment:
            out.update(_alignment_stats(rows, end_slack, gap_min, back_slack))
        if aligned:
            out.update(_aligned_stats(rows))
        if durations:
            out.update(_duration_stats(rows))
        return out
    out = {'overall': stats(records),
           'by_emotion': {name: stats([r for r in records if int(r['emotion']) == i]) for i, name in enumerate(emotions)}}
    if any('style_emotion' in r for r in records):
        out['style'] = _style_block(records, emotions, style_info)
    if any('loudness_shift_lu' in r for r in records):
        out['energy'] = _energy_block(records, emotions)
    if any('alpha_shift_db' in r for r in records):
        out['voice'] = _voice_block(records, emotions)
    return out


def parse_attention_window(text):
    """'BACK,AHEAD' of the command lines -> (back, ahead), two integers >= 0 (`Decoder.attention_window`); ValueError otherwise"""
    parts = str(text).split(',')
    if len(parts) != 2:
        raise ValueError("--attention_window takes BACK,AHEAD, got %r" % (text,))
    back, ahead = (int(x) for x in parts)
    if back < 0 or ahead < 0:
        raise ValueError("--attention_window takes two integers >= 0, got %r" % (text,))
    return back, ahead
