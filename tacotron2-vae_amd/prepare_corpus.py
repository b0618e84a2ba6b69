"""Corpus preparation: a filelist of wavs at any sampling rate becomes a training-ready one — every wav resampled to the
front end's rate, trimmed of leading and trailing silence and written as 16-bit PCM, on the device (t2v_hip.resample,
trim_bounds, crop; csrc/resample.hip).

    python prepare_corpus.py --filelist_path F --out_dir D --out_filelist F2
           [--sampling_rate 16000] [--trim_db 40 | --no_trim] [--pad_frames 2] [--batch_size 64] [--report R.json]
           [--lufs TARGET [--lufs_scope utterance|speaker] [--peak_db -1.0]]
           [--speed_perturb 0.9,1.1] [--pitch_perturb -1,1] [--formant_perturb -1,1] [--preserve_formants]

Filelist rows are `path|text|speaker|emotion` (any column count, the path first).  Each wav is read as it lies in the file
(int16 goes to the device as it is; int32 and float wavs are scaled to [-1, 1) on the host; a wav with more than one channel
is skipped, with its reason in the report), and the rows run in length-sorted ragged batches of at most --batch_size, one
resample launch per distinct source rate in a batch.  D/<basename>.wav is written at the target rate (a basename that
several rows share gets its parent directories prefixed), F2 holds the new paths with the other columns untouched, in the
order of F, without the skipped rows.  The report (R.json, default D/report.json) has per row: source rate, samples in and
out, seconds trimmed at head and tail, peak, clipped samples and the all-silent flag; and totals by source rate.

--lufs TARGET (off by default: without it the written bits and the report are what they were) also normalises the level: the
trimmed wav's integrated loudness (t2v_hip.loudness: ITU-R BS.1770-4 / EBU R 128, K-weighted and gated) is measured and the
wav is scaled (t2v_hip.scale_rows) by TARGET minus that many dB before the 16-bit write-out, so `peak` and `clipped_samples`
describe what is written.  A wav without a loudness (shorter than 400 ms, or below the gates) is written unscaled with
`loudness_lufs: null`.  A gain that would push a wav's peak above --peak_db dBFS is lowered to exactly that (`gain_limited`).
--lufs_scope speaker gives every speaker (filelist column 3) ONE gain, so that the level differences between that speaker's
emotions survive: a first pass measures every row and writes nothing, the speaker's loudness is pooled from the rows' gated
block sums and counts, -0.691 + 10 log10(sum of gated sums / sum of gated counts), and a second pass applies TARGET minus that.
The relative gate stays per row here: it is not that of the speaker's concatenated recordings.  A peak limit lowers the whole
speaker's gain.  The report then has per row `loudness_lufs` (before the gain), `gain_db` and `gain_limited`, per speaker the
pooled loudness and the gain, and in `loudness` the mean and spread of the measured loudness.

--speed_perturb R,... and --pitch_perturb ST,... (off by default; the usual augmentation of a small corpus) add one more copy of
every row per listed value: the resampled and trimmed wav through t2v_hip.time_stretch at the rate R (0.25..4, above 1 is
faster) or t2v_hip.pitch_shift by ST semitones (-12..12), the phase vocoder of csrc/tsm.hip, before the loudness normalisation
and the 16-bit write-out.  A copy is written as D/<stem>_sp0.90.wav / D/<stem>_ps-1.wav and listed in F2 right behind its row,
with the row's other columns.  With --lufs every copy gets its own gain, or its speaker's, lowered where the copy's own peak would pass --peak_db.  The row's record in the report
gains `perturbed`: per copy kind ('speed' or 'pitch'), value, out_path, samples_out, peak, clipped_samples (and the loudness
fields); a row of 512 samples or fewer after the trim has no copies and says so in `perturb_skipped`.  The unperturbed row is
written exactly as without the flags.

--formant_perturb ST,... adds copies with the spectral envelope, the formants, moved by ST semitones and the harmonics in
place (t2v_hip.formant_shift, csrc/envelope.hip), written as D/<stem>_fs-1.wav behind the pitch copies, kind
'formant' in the report: a change of vocal-tract length, another voice at the same pitch.  --preserve_formants makes the
--pitch_perturb copies move F0 alone (t2v_hip.pitch_shift(preserve_formants=True)); without it a pitch copy's formants move
with its pitch, so the speaker drifts with the shift.  The report's `perturbations` gains `formant` and `preserve_formants`
only when one of the two flags is given."""
import argparse
import json
import math
import os

DEFAULT_BATCH_SIZE = 64
DEFAULT_SAMPLING_RATE = 16000
DEFAULT_PEAK_DB = -1.0
LUFS_SCOPES = ('utterance', 'speaker')


def build_arg_parser():
    from wavio import DEFAULT_PAD_FRAMES, DEFAULT_TRIM_DB
    p = argparse.ArgumentParser(description="filelist of wavs at any rate -> resampled, trimmed 16-bit wavs and their filelist")
    p.add_argument('--filelist_path', required=True, help="rows path|... (the wav's path first)")
    p.add_argument('--out_dir', required=True, help="directory of the prepared wavs")
    p.add_argument('--out_filelist', required=True, help="the filelist with the prepared wavs' paths")
    p.add_argument('--sampling_rate', type=int, default=DEFAULT_SAMPLING_RATE, help="target rate in Hz")
    g = p.add_mutually_exclusive_group()
    g.add_argument('--trim_db', type=float, default=DEFAULT_TRIM_DB, metavar='DB',
                   help="trim frames more than DB dB below the wav's loudest frame from both ends")
    g.add_argument('--no_trim', action='store_true', help="resample only")
    p.add_argument('--pad_frames', type=int, default=DEFAULT_PAD_FRAMES, help="frames of 256 samples kept around what sounds")
    p.add_argument('--batch_size', type=int, default=DEFAULT_BATCH_SIZE, help="wavs per ragged batch")
    p.add_argument('--report', default=None, help="report .json (default <out_dir>/report.json)")
    p.add_argument('--lufs', type=float, default=None, metavar='TARGET',
                   help="normalise the integrated loudness (BS.1770) to TARGET LUFS; off by default")
    p.add_argument('--lufs_scope', choices=LUFS_SCOPES, default='utterance',
                   help="one gain per wav, or one per speaker (filelist column 3)")
    p.add_argument('--peak_db', type=float, default=DEFAULT_PEAK_DB, metavar='DB',
                   help="no gain lifts a wav's peak above DB dBFS (<= 0)")
    p.add_argument('--speed_perturb', type=parse_speed_list, default=[], metavar='R,...',
                   help="also write a copy of every wav at each of these tempo rates (0.25..4, not 1); off by default")
    p.add_argument('--pitch_perturb', type=parse_pitch_list, default=[], metavar='ST,...',
                   help="also write a copy of every wav shifted by each of these semitone counts (-12..12, not 0); a list that starts "
                        "with a minus sign may also be written --pitch_perturb=-1,1; off by default")
    p.add_argument('--formant_perturb', type=parse_formant_list, default=[], metavar='ST,...',
                   help="also write a copy of every wav with its formants moved by each of these semitone counts (-12..12, not 0) "
                        "and its pitch kept; off by default")
    p.add_argument('--preserve_formants', action='store_true',
                   help="the --pitch_perturb copies keep their formants in place (F0 alone moves); off by default")
    return p


def _number_list(text, what, check, identity):
    import t2v_hip
    try:
        values = [float(x) for x in text.split(',') if x.strip()]
        for v in values:
            getattr(t2v_hip, check)(v)
    except ValueError as e:
        raise argparse.ArgumentTypeError("%s: %s" % (what, e))
    if not values or identity in values or len(set(values)) != len(values):
        raise argparse.ArgumentTypeError("%s takes distinct comma separated values other than %g, got %r" % (what, identity, text))
    return values


def parse_speed_list(text):
    """'0.9,1.1' -> [0.9, 1.1]: tempo rates in 0.25..4, distinct, none of them 1"""
    return _number_list(text, '--speed_perturb', 'stretch_ratio', 1.0)


def parse_pitch_list(text):
    """'-1,1' -> [-1.0, 1.0]: semitones in -12..12, distinct, none of them 0"""
    return _number_list(text, '--pitch_perturb', 'pitch_ratio', 0.0)


def parse_formant_list(text):
    """'-1,1' -> [-1.0, 1.0]: semitones in -12..12, distinct, none of them 0"""
    return _number_list(text, '--formant_perturb', 'pitch_ratio', 0.0)


def perturbed_name(name, kind, value):
    """the file name of a perturbed copy of <stem>.wav: <stem>_sp0.90.wav for a tempo rate, <stem>_ps-1.wav / <stem>_ps1.5.wav
    for a pitch shift in semitones, <stem>_fs-1.wav for a formant shift"""
    stem = name[:-4] if name.lower().endswith('.wav') else name
    if kind == 'speed':
        return "%s_sp%.2f.wav" % (stem, value)
    if kind in ('pitch', 'formant'):
        return "%s_%s%s.wav" % (stem, 'ps' if kind == 'pitch' else 'fs', "%d" % value if float(value) == int(value) else "%g" % value)
    raise ValueError("perturbed_name: kind must be 'speed', 'pitch' or 'formant', got %r" % (kind,))


def parse_args(argv=None):
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    for k in range(len(argv) - 2, -1, -1):    # "--pitch_perturb -1,1": argparse takes a list that starts with '-' for a flag
        if argv[k] in ('--pitch_perturb', '--speed_perturb', '--formant_perturb') and argv[k + 1][:1] == '-' and argv[k + 1][1:2].isdigit():
            argv[k:k + 2] = [argv[k] + '=' + argv[k + 1]]
    args = build_arg_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    if args.sampling_rate < 1:
        raise SystemExit("--sampling_rate must be >= 1")
    if args.pad_frames < 0:
        raise SystemExit("--pad_frames must be >= 0")
    if not args.no_trim and not 0.0 < args.trim_db < float('inf'):
        raise SystemExit("--trim_db must be a positive number of dB")
    if not args.peak_db <= 0.0 or math.isinf(args.peak_db):
        raise SystemExit("--peak_db must be a finite level <= 0 dBFS")
    if args.lufs is not None and not math.isfinite(args.lufs):
        raise SystemExit("--lufs must be a finite level in LUFS")
    tags = [perturbed_name('x.wav', 'speed', v) for v in args.speed_perturb] + [perturbed_name('x.wav', 'pitch', v) for v in args.pitch_perturb]
    tags += [perturbed_name('x.wav', 'formant', v) for v in args.formant_perturb]
    if len(set(tags)) != len(tags):
        raise SystemExit("--speed_perturb / --pitch_perturb / --formant_perturb: two values give one file name (%s)"
                         % ', '.join(sorted(tags)))
    if args.preserve_formants and not args.pitch_perturb:
        raise SystemExit("--preserve_formants changes the --pitch_perturb copies: give --pitch_perturb")
    if args.report is None:
        args.report = os.path.join(args.out_dir, 'report.json')
    return args


def gain_for(target, loudness, peak, peak_db=DEFAULT_PEAK_DB):
    """(gain in dB, limited) that brings `loudness` (LUFS; None or -inf: no loudness, gain 0) to `target`, lowered to exactly
    peak_db - 20 log10(peak) where it would lift the peak (linear, of the same samples) above peak_db dBFS"""
    if loudness is None or math.isinf(loudness) or math.isnan(loudness):
        return 0.0, False
    gain = float(target) - float(loudness)
    if peak > 0.0:
        room = float(peak_db) - 20.0 * math.log10(peak)
        if gain > room:
            return room, True
    return gain, False


def pooled_loudness(gated_sums, gated_blocks):
    """-0.691 + 10 log10(sum of the rows' gated block sums / sum of their gated block counts); None without a gated block"""
    total, count = sum(gated_sums), sum(gated_blocks)
    return -0.691 + 10.0 * math.log10(total / count) if count > 0 and total > 0.0 else None


def speaker_gains(rows, target, peak_db=DEFAULT_PEAK_DB):
    """rows: (speaker, gated_sum, gated_blocks, peak) per measured wav.  {speaker: dict(loudness_lufs, gain_db, gain_limited,
    rows)}: the pooled loudness of the speaker's rows, and target minus it, limited by the speaker's largest peak, so that one
    gain serves all the speaker's rows; a speaker without a gated block keeps gain 0 and loudness None."""
    by = {}
    for speaker, gsum, gcount, peak in rows:
        t = by.setdefault(speaker, dict(sums=[], counts=[], peak=0.0))
        t['sums'].append(gsum)
        t['counts'].append(gcount)
        t['peak'] = max(t['peak'], peak)
    out = {}
    for speaker, t in by.items():
        loud = pooled_loudness(t['sums'], t['counts'])
        gain, limited = gain_for(target, loud, t['peak'], peak_db)
        out[speaker] = dict(loudness_lufs=loud, gain_db=gain, gain_limited=limited, rows=len(t['sums']))
    return out


def loudness_totals(records):
    """mean and spread (standard deviation) of the measured loudness over the written rows that have one"""
    v = [r['loudness_lufs'] for r in records if not r.get('skipped') and r.get('loudness_lufs') is not None]
    if not v:
        return dict(rows=0, mean_lufs=None, spread_lu=None)
    mean = sum(v) / len(v)
    return dict(rows=len(v), mean_lufs=mean, spread_lu=math.sqrt(sum((x - mean) ** 2 for x in v) / len(v)))


def read_rows(path):
    """the rows of a filelist as lists of columns (path first), blank lines dropped"""
    with open(path, encoding='utf-8') as f:
        return [line.rstrip('\r\n').split('|') for line in f if line.strip()]


def output_names(paths):
    """<basename>.wav for every path, unique: a basename that several paths share gets as many parent directories prefixed
    (joined by '_') as it takes to tell them apart, and what still collides (the same path twice) a running number"""
    def parts(p):
        p = os.path.normpath(p)
        stem = os.path.splitext(os.path.basename(p))[0]
        dirs = [d for d in os.path.dirname(p).split(os.sep) if d not in ('', '.')]
        return dirs, stem

    split = [parts(p) for p in paths]
    depth = [0] * len(paths)

    def name(i):
        dirs, stem = split[i]
        return '_'.join(dirs[len(dirs) - depth[i]:] + [stem]) if depth[i] else stem

    while True:
        seen = {}
        for i in range(len(paths)):
            seen.setdefault(name(i), []).append(i)
        grew = False
        for idx in seen.values():
            if len(idx) > 1:
                for i in idx:
                    if depth[i] < len(split[i][0]):
                        depth[i] += 1
                        grew = True
        if not grew:
            break
    out, used = [], {}
    for i in range(len(paths)):
        base = name(i)
        k = used.get(base, 0)
        used[base] = k + 1
        out.append((base if k == 0 else "%s_%d" % (base, k)) + '.wav')
    if len(set(out)) != len(out):        # a running number that meets another row's own name
        out = ["%06d_%s" % (i, n) for i, n in enumerate(out)]
    return out


def rewrite_rows(rows, new_paths):
    """the rows with their first column replaced (None: the row is dropped), as filelist lines"""
    return ['|'.join([p] + list(r[1:])) for r, p in zip(rows, new_paths) if p is not None]


def summarize(records):
    """totals by source rate of the per-row records"""
    by_rate = {}
    for r in records:
        if r.get('skipped'):
            continue
        t = by_rate.setdefault(str(r['source_rate']), dict(rows=0, seconds_in=0.0, seconds_out=0.0, seconds_trimmed=0.0,
                                                           clipped_samples=0, all_silent=0, peak_max=0.0))
        t['rows'] += 1
        t['seconds_in'] += r['samples_in'] / float(r['source_rate'])
        t['seconds_out'] += r['samples_out'] / float(r['target_rate'])
        t['seconds_trimmed'] += r['trimmed_head_s'] + r['trimmed_tail_s']
        t['clipped_samples'] += r['clipped_samples']
        t['all_silent'] += int(r['all_silent'])
        t['peak_max'] = max(t['peak_max'], r['peak'])
    return by_rate


def front_end(items, target_rate, trim_db, pad_frames):
    """items: [(source rate, samples (int16 or float32 numpy))].  Returns (y (B, max count) float32 on the device, the resampled
    counts, the (start, end) each row is to be cropped to): resample (one launch per distinct (rate, format)) -> trim_bounds
    of one ragged batch.  No caller writes into y, so one result serves the plain row and its perturbed copies."""
    import t2v_hip
    from synthesizer import resample_rows
    y, n = resample_rows(items, target_rate)
    if trim_db is None:
        bounds = [[0, k] for k in n]
    else:
        bounds = t2v_hip.trim_bounds(y, n, trim_db, pad_frames).cpu().tolist()
    return y, n, bounds


def process_batch(items, target_rate, trim_db, pad_frames, front=None):
    """Returns per item (int16 numpy samples, record fields): front_end (or its result `front`, when the caller has it) -> crop
    to int16, as one ragged batch."""
    import t2v_hip
    y, n, bounds = front or front_end(items, target_rate, trim_db, pad_frames)
    pcm, counts, stats = t2v_hip.crop(y, bounds, pcm16=True, return_stats=True)
    pcm = pcm.cpu().numpy()
    out = []
    for b, (rate, data) in enumerate(items):
        start, end = bounds[b]
        clipped, peak = stats[b]
        out.append((pcm[b, :counts[b]].copy(),
                    dict(source_rate=rate, target_rate=target_rate, samples_in=int(len(data)), samples_resampled=n[b],
                         samples_out=counts[b], trimmed_head_s=start / float(target_rate),
                         trimmed_tail_s=(n[b] - end) / float(target_rate), peak=peak, clipped_samples=clipped,
                         all_silent=bool(peak == 0.0))))
    return out


def measure_batch(items, target_rate, trim_db, pad_frames, front=None):
    """front_end (or its result `front`) -> crop (fp32) -> loudness of one ragged batch.  Returns (y (B, max count) float32 on
    the device, counts, per-item record fields without the write-out's, per-item (integrated LUFS or None, gated_sum,
    gated_blocks, peak))."""
    import t2v_hip
    y, n, bounds = front or front_end(items, target_rate, trim_db, pad_frames)
    y, counts = t2v_hip.crop(y, bounds)
    loud = t2v_hip.loudness(y, [max(c, 1) for c in counts], target_rate)
    peaks = y.abs().amax(dim=1).tolist()
    fields, measured = [], []
    for b, (rate, data) in enumerate(items):
        start, end = bounds[b]
        fields.append(dict(source_rate=rate, target_rate=target_rate, samples_in=int(len(data)), samples_resampled=n[b],
                           samples_out=counts[b], trimmed_head_s=start / float(target_rate),
                           trimmed_tail_s=(n[b] - end) / float(target_rate)))
        lu = loud.integrated[b]
        measured.append((None if math.isinf(lu) else lu, loud.gated_sum[b], loud.gated_blocks[b], float(peaks[b])))
    return y, counts, fields, measured


def process_batch_lufs(items, target_rate, trim_db, pad_frames, target, peak_db, gains=None, front=None):
    """process_batch with the level normalised: measure_batch -> gain -> scale_rows -> crop to int16.  gains: one
    (gain_db, limited) per item (the speaker's), or None for each row's own, gain_for(target, its loudness, its peak)."""
    import t2v_hip
    y, counts, fields, measured = measure_batch(items, target_rate, trim_db, pad_frames, front)
    if gains is None:
        gains = [gain_for(target, lu, peak, peak_db) for lu, _, _, peak in measured]
    lengths = [max(c, 1) for c in counts]
    t2v_hip.scale_rows(y, lengths, [10.0 ** (g / 20.0) for g, _ in gains])
    pcm, counts, stats = t2v_hip.crop(y, [[0, c] for c in counts], pcm16=True, return_stats=True)
    pcm = pcm.cpu().numpy()
    out = []
    for b in range(len(items)):
        clipped, peak = stats[b]
        out.append((pcm[b, :counts[b]].copy(),
                    dict(fields[b], peak=peak, clipped_samples=clipped, all_silent=bool(peak == 0.0),
                         loudness_lufs=measured[b][0], gain_db=gains[b][0], gain_limited=gains[b][1])))
    return out


PERTURB_MIN_SAMPLES = 513                # the phase vocoder's transform reflect-pads by 512


def process_batch_perturbed(front, target_rate, variants, target=None, peak_db=DEFAULT_PEAK_DB, gains=None, preserve_formants=False):
    """The perturbed copies of one ragged batch, from the front_end result the plain rows were written from: crop (fp32), then
    per variant (kind, value) time_stretch, pitch_shift (with preserve_formants: F0 alone) or formant_shift of the rows that are
    long enough, with a target the level
    normalisation of process_batch_lufs, and the crop to int16.  gains: None for each copy's own, or one (gain_db, limited) per
    item, the speaker's; that gain was limited by the peaks of the unperturbed rows, and a copy may overshoot them, so it is
    lowered for a copy whose own peak it would lift above peak_db (`gain_limited` on that copy).  Returns per item None (512
    samples or fewer) or a list, in the order of the variants, of (int16 numpy samples, record fields)."""
    import torch
    import t2v_hip
    y, counts = t2v_hip.crop(front[0], front[2])
    can = [b for b, c in enumerate(counts) if c >= PERTURB_MIN_SAMPLES]
    out = [None] * len(counts)
    if not can:
        return out
    if len(can) < len(out):
        y = y[torch.tensor(can, device=y.device)].contiguous()
    counts = [counts[b] for b in can]
    for b in can:
        out[b] = []
    for kind, value in variants:
        if kind == 'speed':
            z, m = t2v_hip.time_stretch(y, counts, value)
        elif kind == 'formant':
            z, m = t2v_hip.formant_shift(y, counts, value)
        else:
            z, m = t2v_hip.pitch_shift(y, counts, value, preserve_formants=preserve_formants)
        extra = [{} for _ in can]
        if target is not None:
            z = z.clone() if z is y else z
            loud = t2v_hip.loudness(z, m, target_rate)
            peaks = z.abs().amax(dim=1).tolist()
            lus = [None if math.isinf(lu) else lu for lu in loud.integrated]
            if gains is None:
                g = [gain_for(target, lu, pk, peak_db) for lu, pk in zip(lus, peaks)]
            else:
                g = []
                for b, pk in zip(can, peaks):
                    room = float(peak_db) - 20.0 * math.log10(pk) if pk > 0.0 else float('inf')
                    g.append((room, True) if gains[b][0] > room else gains[b])
            t2v_hip.scale_rows(z, m, [10.0 ** (x / 20.0) for x, _ in g])
            extra = [dict(loudness_lufs=lu, gain_db=x, gain_limited=lim) for lu, (x, lim) in zip(lus, g)]
        pcm, m, stats = t2v_hip.crop(z, [[0, k] for k in m], pcm16=True, return_stats=True)
        pcm = pcm.cpu().numpy()
        for k, b in enumerate(can):
            clipped, peak = stats[k]
            out[b].append((pcm[k, :m[k]].copy(), dict(extra[k], kind=kind, value=value, samples_out=m[k], peak=peak,
                                                     clipped_samples=clipped)))
    return out


def main(argv=None):
    args = parse_args(argv)
    from scipy.io.wavfile import write
    import t2v_hip
    from synthesizer import length_groups
    from wavio import read_wav, wav_header
    rows = read_rows(args.filelist_path)
    if not rows:
        raise SystemExit("%s: no rows" % args.filelist_path)
    by_speaker = args.lufs is not None and args.lufs_scope == 'speaker'
    if args.lufs is not None:
        try:
            t2v_hip.kweight_coefficients(args.sampling_rate)
        except ValueError as e:
            raise SystemExit("--lufs: %s" % e)
    if by_speaker and any(len(r) < 3 for r in rows):
        raise SystemExit("%s: --lufs_scope speaker needs the speaker in a third column (path|text|speaker|...)"
                         % args.filelist_path)
    os.makedirs(args.out_dir, exist_ok=True)
    names = output_names([r[0] for r in rows])
    records = [None] * len(rows)
    lengths, keep = [], []
    for i, r in enumerate(rows):
        try:
            rate, count, channels = wav_header(r[0])
            if channels != 1:
                raise ValueError("%d channels; only mono wavs are prepared" % channels)
            if count < 1:
                raise ValueError("no samples")
            t2v_hip.resample_taps(rate, args.sampling_rate)             # a ratio outside the table limit is this row's reason
            lengths.append(t2v_hip.resample_length(count, *t2v_hip.resample_ratio(rate, args.sampling_rate)))
            keep.append(i)
        except (ValueError, OSError) as e:
            records[i] = dict(path=r[0], skipped=str(e))
    new_paths = [None] * len(rows)
    trim_db = None if args.no_trim else args.trim_db
    variants = [('speed', v) for v in args.speed_perturb] + [('pitch', v) for v in args.pitch_perturb]
    variants += [('formant', v) for v in args.formant_perturb]
    copies = [[] for _ in rows]                                          # the perturbed copies' paths, per row

    def batches():
        for idx in length_groups(lengths, args.batch_size):
            group, items = [], []
            for k in idx:
                i = keep[k]
                if records[i] is not None and records[i].get('skipped'):
                    continue
                try:
                    items.append(read_wav(rows[i][0]))
                    group.append(i)
                except (ValueError, OSError) as e:
                    records[i] = dict(path=rows[i][0], skipped=str(e))
            if items:
                yield group, items

    speakers = None
    if by_speaker:                                                       # first pass: measure every row, write nothing
        measured = []
        for group, items in batches():
            for i, m in zip(group, measure_batch(items, args.sampling_rate, trim_db, args.pad_frames)[3]):
                measured.append((rows[i][2], m[1], m[2], m[3]))
        speakers = speaker_gains(measured, args.lufs, args.peak_db)
    for group, items in batches():
        front = front_end(items, args.sampling_rate, trim_db, args.pad_frames) if variants else None
        if args.lufs is None:
            done = process_batch(items, args.sampling_rate, trim_db, args.pad_frames, front)
        else:
            gains = [(speakers[rows[i][2]]['gain_db'], speakers[rows[i][2]]['gain_limited']) for i in group] if by_speaker else None
            done = process_batch_lufs(items, args.sampling_rate, trim_db, args.pad_frames, args.lufs, args.peak_db, gains, front)
        for i, (pcm, rec) in zip(group, done):
            new_paths[i] = os.path.join(args.out_dir, names[i])
            write(new_paths[i], args.sampling_rate, pcm)
            records[i] = dict(rec, path=rows[i][0], out_path=new_paths[i])
        if variants:
            done = process_batch_perturbed(front, args.sampling_rate, variants, args.lufs, args.peak_db,
                                           gains if args.lufs is not None else None, args.preserve_formants)
            for i, made in zip(group, done):
                records[i]['perturbed'] = []
                if made is None:
                    records[i]['perturb_skipped'] = "%d samples or fewer after the trim" % (PERTURB_MIN_SAMPLES - 1)
                    continue
                for pcm, rec in made:
                    path = os.path.join(args.out_dir, perturbed_name(names[i], rec['kind'], rec['value']))
                    write(path, args.sampling_rate, pcm)
                    copies[i].append(path)
                    records[i]['perturbed'].append(dict(rec, out_path=path))
    with open(args.out_filelist, 'w', encoding='utf-8') as f:
        for r, p, extra in zip(rows, new_paths, copies):
            for line in rewrite_rows([r] * (1 + len(extra)), [p] + extra):
                f.write(line + '\n')
    n_skipped = sum(1 for r in records if r.get('skipped'))
    report = dict(target_rate=args.sampling_rate, trim_db=None if args.no_trim else args.trim_db, pad_frames=args.pad_frames,
                  n_rows=len(rows), n_written=len(rows) - n_skipped, n_skipped=n_skipped, by_source_rate=summarize(records),
                  rows=records)
    if variants:
        report['perturbations'] = dict(speed=args.speed_perturb, pitch=args.pitch_perturb,
                                       n_written=sum(len(c) for c in copies))
        if args.formant_perturb or args.preserve_formants:
            report['perturbations'].update(formant=args.formant_perturb, preserve_formants=args.preserve_formants)
    if args.lufs is not None:
        report['loudness'] = dict(loudness_totals(records), target_lufs=args.lufs, scope=args.lufs_scope, peak_db=args.peak_db)
        if speakers is not None:
            report['speakers'] = speakers
    with open(args.report, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    print("%s: %d wavs at %d Hz, %d skipped; %s" % (args.out_filelist, len(rows) - n_skipped, args.sampling_rate, n_skipped,
                                                   args.report))
    return report


if __name__ == "__main__":
    main()
