"""Score a checkpoint by free-running synthesis: every utterance of a filelist is synthesised from its text and compared
with its own recording by mel-spectral distortion with dynamic time warping (`Synthesizer.evaluate`, csrc/dtw.hip).

    python evaluate.py --load_path CKPT --filelist_path F --out OUT.json
                       [--batch_size N] [--condition ref|emotion] [--limit N] [--prosody] [--alignment]
                       [--style [--style_k K]] [--aligned] [--energy] [--voice] [--durations [--max_step S]] [--attention_window BACK,AHEAD] [--rhythm ref [--rhythm_window BACK,AHEAD]] [--weights raw|ema] [--speed R]
                       [--pitch ST] [--formant ST] [--preserve_formants]
                       [--hparams ...]

Filelist rows are `path|text|speaker|emotion`.  --condition ref (default) takes the style from the row's own recording
(copy synthesis); --condition emotion takes the centroid of the row's emotion label (built from the filelist, or read from
its cache next to the checkpoint).  OUT.json holds {"summary": evaluation.summarize(rows), "rows": [...]}, row i for
filelist row i: path, dtw, n_frames, n_ref_frames, hit_max, emotion.

--prosody also asks whether the synthesised speech carries the style's pitch.  The checkpoint is loaded with the Griffin-Lim
vocoder; each synthesised mel becomes a waveform, and a YIN pitch track (`t2v_hip.f0`, csrc/f0.hip: 60-500 Hz, one value per
mel frame) is taken of it and of the recording.  Every row gains f0_median_hz / f0_ref_median_hz (median over voiced
frames), f0_spread_st / f0_ref_spread_st (standard deviation of the pitch around that median, in semitones: the pitch
range), voiced_share / voiced_ref_share and f0_shift_st (semitones from the recording's median to the synthesis's); the
F0 values are null for a side with fewer than 5 voiced frames.  Every summary dict gains n_prosody (rows that stopped at the
gate and have a shift), f0_shift_st_mean (signed), f0_shift_st_abs_mean, f0_spread_ratio_mean (synthesised spread over the
recording's: far below 1 is a flat voice, which a DTW mel distance hardly sees), voiced_share_mean and
voiced_ref_share_mean.  Mel -> Griffin-Lim itself moves a median by about 0.1 semitone (up to 0.3 measured on steady
tones), and a steady pitch below 140 Hz can come back unvoiced.

--alignment asks whether the decoder read the sentence: a skipped or repeated word, attention stuck on one symbol or a stop
before the end of the text show in the attention alignment and nowhere else.  The alignments the decoder already returns are
reduced on the device (`t2v_hip.alignment_stats`, csrc/align.hip); p[t] is the text position frame t attends most.  Every row
gains focus (mean weight on p[t]), reach ((furthest p + 1) / symbols), end_reach ((p of the last frame + 1) / symbols),
back_share and jump_share (steps back, and forward by more than 3 positions, over the transitions), stall_frames (longest run
of frames on one position), uncovered_share (symbols whose summed weight stays under 0.5), gap_symbols (longest run of such
symbols) and n_symbols.  Every summary dict gains, over the n_alignment rows that stopped at the gate, focus_mean, reach_mean,
back_share_mean, jump_share_mean, uncovered_share_mean, stall_frames_mean / _max, gap_symbols_mean / _max, n_read_through and
read_through_share: a row reads through when its last frame attends one of the last 4 symbols, fewer than 4 consecutive
symbols stay uncovered and at most 2 steps go back.  These thresholds are choices, not calibrated on a trained model
(DESIGN 7h); the per-row numbers are always written, so they can be cut again (evaluation.summarize takes the thresholds).

--style asks whether the decoder obeys the latent: a collapsed posterior, or a decoder that ignores the style it is given,
hardly moves a DTW mel distance.  Every synthesised mel is encoded again (the ragged `model.vae_gst`), and its mu is placed
among the mu of the filelist's distinct recordings, labelled with their emotions (`t2v_hip.latent_neighbours`,
csrc/latent.hip), the row's own recording left out of the vote.  Every row gains style_emotion (the vote of the --style_k
nearest other recordings), style_hit (it equals the row's label), style_own_rank (how many recordings lie closer than the
row's own: 0 means the synthesis is nearest to the clip it copied, the retrieval reading under --condition ref; it is written
under --condition emotion too), style_own_dist and style_silhouette (against the recorded clusters); null for a row decoded
to fewer than 2 frames.  The summary gains "style": per emotion and overall accuracy, rank0_share, rank_median and
silhouette_mean, the 4 x 4 confusion matrix, and ref_accuracy, the leave-one-out accuracy of the recordings themselves under
the same k: the ceiling the synthesised accuracy has to be read against.  One path under two emotion labels, or fewer than 2
distinct recordings, is an error; --style_k is lowered to (distinct recordings - 1) when there are too few.

--aligned gives the frame-aligned numbers the prosody-transfer papers report.  Both mels are reduced to 13 mel-cepstral
coefficients (the DCT of the 80-band log-mel, c_0 left out: the papers' MCD-13, not a vocoder's mel-generalised cepstrum), a DTW
over them that keeps its decisions gives the warping path (`t2v_hip.aligned_scores`, csrc/aligned.hip), and the scores are
taken over the path's points.  Every row gains mcd_db and warp_dev (mean |i / (Tx - 1) - j / (Ty - 1)| along the path: 0 when the
synthesis is a linear stretch of the recording, so it scores the speaking rhythm).  With --prosody the two pitch tracks feed
the same call and the row also gains vde (voicing decision error), gpe (gross pitch error: more than 20 % apart where both
sides are voiced), ffe (F0 frame error: either), lf0_rmse_cents, lf0_bias_cents and lf0_corr; without it those six are null, and
no vocoder is needed.  Every summary dict gains n_aligned (rows that stopped at the gate) and mcd_db_mean, vde_mean, gpe_mean,
ffe_mean, lf0_rmse_cents_mean, lf0_corr_mean and warp_dev_mean, each over the rows that have the value.

--energy asks about the third correlate of prosody, the level: does an "ang" row come out louder than a "sad" one, as the
recordings do?  The checkpoint is loaded with the Griffin-Lim vocoder (as for --prosody, which shares the waveforms), and the
K-weighted, gated loudness of ITU-R BS.1770-4 and the K-weighted level per mel frame (`t2v_hip.loudness`, csrc/loudness.hip)
are taken of each synthesised waveform and of its recording.  Every row gains loudness_lufs, loudness_ref_lufs,
loudness_shift_lu (synthesis - recording) and energy_spread_db / energy_ref_spread_db (standard deviation of the frame level
over the frames within 40 dB of the row's loudest: an uncalibrated choice); null for a side without a loudness (no waveform,
under 400 ms, or below the gates).  With --aligned the row also gains energy_rmse_db and energy_corr of the two dB tracks
along the warping path, over the points where both sides sound.  The summary gains "energy": overall and per emotion n_energy,
loudness_shift_lu_mean / _abs_mean, energy_spread_ratio_mean (and the two path means), and per emotion loudness_vs_neu_lu and
loudness_ref_vs_neu_lu, the emotion's mean loudness minus neutral's, synthesised and recorded.

--voice asks about the fourth correlate, voice quality: is an "ang" row pressed (a flat spectral tilt) and a "sad" one lax and
breathy (a steep tilt, a weak cepstral peak), as the recordings are?  A decoder can copy a clip's pitch and level and still
render every emotion with the neutral voice's timbre.  On the same two waveforms as --prosody and --energy, the spectral-balance
descriptors of eGeMAPS and the cepstral peak prominence are taken per mel frame (`t2v_hip.voice_quality`, csrc/voice.hip).
Every row gains alpha_db / alpha_ref_db (1-5 kHz over 50 Hz-1 kHz), hammarberg_db / hammarberg_ref_db (the peak below 2 kHz
over the peak in 2-5 kHz), slope_db_khz / slope_ref_db_khz (500-1500 Hz), cpp_db / cpp_ref_db and alpha_shift_db, cpp_shift_db
(synthesis - recording), each the median over the frames that are not silent and lie within 40 dB of the row's loudest; null
for a side without such a frame or without a waveform.  With --aligned the row also gains alpha_rmse_db and alpha_corr of the
two alpha_db tracks along the warping path.  The summary gains "voice": overall and per emotion n_voice and the means of the
keys, and per emotion alpha_vs_neu_db, alpha_ref_vs_neu_db, cpp_vs_neu_db and cpp_ref_vs_neu_db, the emotion's mean minus
neutral's, synthesised and recorded; no thresholds.

--durations asks about timing per symbol, which warp_dev gives as one number per utterance.  The best monotonic path through
an alignment matrix (`t2v_hip.mas`, csrc/durations.hip: monotonic alignment search, steps of at most --max_step symbols per
frame) says that symbol j occupies the frames [s, e).  It is run on the free-running alignments of the synthesis and on the
teacher-forced alignments of the recording against the same text (one forward per row), so both sides are segmented into the
text's own symbols.  Every row gains dur_rmse_frames, dur_corr (Pearson over the symbols), dur_log_ratio_spread (standard
deviation of ln((1 + d_syn) / (1 + d_rec)): 0 for a uniform change of tempo), align_logp_syn and align_logp_rec (the mean log
weight along each path: low where text and audio do not match); with --prosody also seg_f0_rmse_cents and seg_f0_corr, of the
mean F0 per symbol over the symbols voiced on both sides.  A side whose text has more symbols than its frames can reach has
null.  Every summary dict gains n_durations and the means; OUT.json then holds "max_step".  --durations with --prosody is
refused together with --speed / --pitch, as --aligned is.

--attention_window BACK,AHEAD decodes every row under the attention constraint of `Decoder.attention_window` (each frame
attends within BACK positions behind and AHEAD in front of the position the previous frame attended most).
OUT.json always holds "attention_window": [BACK, AHEAD], or null without the flag, so that two reports can be told apart.

--rhythm ref gives every synthesis the rhythm of its own recording: the recording's symbol durations, found by the forced
alignment of --durations, become the decoder's plan (`Synthesizer.evaluate(rows, rhythm='ref')`), and every frame
attends within --rhythm_window BACK,AHEAD (default 1,1) of its planned symbol.  The synthesis then has the recording's frame
count, so what remains in dtw, mcd_db or the F0 errors is not timing.  Every row gains "rhythm"; OUT.json holds "rhythm" and
"rhythm_window" only when the flag is given.

--weights ema scores the averaged weights of the checkpoint ('ema_state_dict', written by a training run with
hparams.ema_decay > 0) instead of the last iteration's; with --condition emotion the centroid cache is a file of its own.
OUT.json always holds "weights": "raw" or "ema".

--speed R and --pitch ST set the tempo and the pitch shift (semitones) of the vocoder leg (`GriffinLimVocoder(speed=, pitch=)`,
DESIGN 7o): the waveforms that --prosody, --energy and --voice measure are the ones the synthesis command line would write
with the same flags, and their tracks run over those waveforms' own frames (ceil(n_frames / speed) of them, not n_frames).
The mels, and with them dtw and every score taken of mels, do not change.  --aligned together with --prosody, --energy or
--voice is refused with them: the warping path is over mel frames, and the waveform's frames lie on another time axis.
OUT.json always holds "speed" and "pitch" (1.0 and 0.0 without the flags).

--formant ST and --preserve_formants act in the same vocoder leg (`GriffinLimVocoder(formant=, preserve_formants=)`, DESIGN
7p): the spectral envelope of the waveform moves by ST semitones with the harmonics in place, and --pitch moves F0 alone.
OUT.json holds "formant" and "preserve_formants" only when one of the two flags is given."""
import argparse
import json

DEFAULT_BATCH_SIZE = 8
DEFAULT_STYLE_K = 5
DEFAULT_MAX_STEP = 1
CONDITIONS = ('ref', 'emotion')


def build_arg_parser():
    p = argparse.ArgumentParser(description="filelist -> DTW mel distance of free-running synthesis per utterance (.json)")
    p.add_argument('--load_path', required=True, help="checkpoint written by train.py")
    p.add_argument('--filelist_path', required=True, help="rows path|text|speaker|emotion")
    p.add_argument('--out', required=True, help="output .json")
    p.add_argument('--batch_size', type=int, default=DEFAULT_BATCH_SIZE, help="rows per synthesize_batch / mel_dtw call")
    p.add_argument('--condition', choices=CONDITIONS, default='ref', help="style from the row's recording or its emotion centroid")
    p.add_argument('--limit', type=int, default=None, help="score only the first N rows")
    p.add_argument('--prosody', action='store_true',
                   help="also track the pitch (YIN, 60-500 Hz) of each synthesised waveform (Griffin-Lim) and of its recording: "
                        "rows gain median F0, spread in semitones, voiced share and f0_shift_st; the summary their means")
    p.add_argument('--vocoder', choices=['griffin_lim', 'griffin_lim_fast', 'spsi'], default='griffin_lim',
                   help="the vocoder of --prosody, --energy and --voice (griffin_lim_fast: momentum 0.99 and NNLS mel inversion; spsi: NNLS "
                        "and the phase from the magnitudes' peaks, no iterations, which keeps low voices voiced); unused "
                        "without them")
    p.add_argument('--alignment', action='store_true',
                   help="also score the attention alignment of each synthesis (did the decoder read the text?): rows gain focus, "
                        "reach, end_reach, back_share, jump_share, stall_frames, uncovered_share, gap_symbols and n_symbols; "
                        "the summary their means and read_through_share")
    p.add_argument('--style', action='store_true',
                   help="also encode each synthesis again and place its mu among the recordings' (style round trip): rows gain "
                        "style_emotion, style_hit, style_own_rank, style_own_dist and style_silhouette; the summary a style block")
    p.add_argument('--style_k', type=int, default=DEFAULT_STYLE_K, help="neighbours of the --style vote; unused without it")
    p.add_argument('--aligned', action='store_true',
                   help="also walk the DTW path over 13 mel-cepstral coefficients and score along it: rows gain mcd_db and "
                        "warp_dev, and with --prosody vde, gpe, ffe, lf0_rmse_cents, lf0_bias_cents and lf0_corr; the summary "
                        "their means")
    p.add_argument('--energy', action='store_true',
                   help="also measure the BS.1770 loudness and the frame level of each synthesised waveform (Griffin-Lim) and of "
                        "its recording: rows gain loudness_lufs, loudness_ref_lufs, loudness_shift_lu and the energy spreads, "
                        "with --aligned energy_rmse_db and energy_corr; the summary an energy block")
    p.add_argument('--voice', action='store_true',
                   help="also measure the voice quality of each synthesised waveform (Griffin-Lim) and of its recording: rows gain "
                        "the medians of alpha ratio, Hammarberg index, spectral slope and cepstral peak prominence on both sides, "
                        "alpha_shift_db and cpp_shift_db, with --aligned alpha_rmse_db and alpha_corr; the summary a voice block")
    p.add_argument('--durations', action='store_true',
                   help="also force the alignments of each synthesis and of its recording (teacher-forced) onto the text by "
                        "monotonic search and compare the frames per symbol: rows gain dur_rmse_frames, dur_corr, "
                        "dur_log_ratio_spread, align_logp_syn and align_logp_rec, with --prosody seg_f0_rmse_cents and "
                        "seg_f0_corr; the summary their means")
    p.add_argument('--max_step', type=int, default=DEFAULT_MAX_STEP, metavar='S',
                   help="symbols the --durations path may advance per frame, 1..3 (above 1 a symbol may be skipped); unused "
                        "without it")
    from evaluation import parse_attention_window
    p.add_argument('--attention_window', type=parse_attention_window, default=None, metavar='BACK,AHEAD',
                   help="attention constraint of the free-running decode: every frame attends within BACK positions behind and "
                        "AHEAD in front of the position the previous frame attended most; written into the report")
    p.add_argument('--rhythm', choices=['ref'], default=None,
                   help="decode every synthesis along the symbol durations of its own recording (forced alignment), which takes "
                        "rhythm out of the comparison; written into the report")
    p.add_argument('--rhythm_window', type=parse_attention_window, default=None, metavar='BACK,AHEAD',
                   help="positions the decoder may look behind and in front of the planned symbol under --rhythm (default 1,1, "
                        "an uncalibrated choice)")
    p.add_argument('--hparams', default='', help="comma separated name=value overrides")
    from wavio import add_wav_arguments
    add_wav_arguments(p)
    from synthesizer import add_tempo_arguments, add_weights_argument
    add_tempo_arguments(p)
    add_weights_argument(p)
    return p


def parse_args(argv=None):
    args = build_arg_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    if not 1 <= args.style_k <= 32:
        raise SystemExit("--style_k must be in 1..32")
    if args.limit is not None and args.limit < 1:
        raise SystemExit("--limit must be >= 1")
    if not 1 <= args.max_step <= 3:
        raise SystemExit("--max_step must be in 1..3")
    if args.durations and args.prosody and (args.speed != 1.0 or args.pitch != 0.0):
        raise SystemExit("--durations with --prosody reads the pitch track over the frames of the alignments' path; with --speed / "
                         "--pitch the waveform is on another time axis: drop one of the two or the tempo flags")
    if args.aligned and (args.prosody or args.energy or args.voice) and (args.speed != 1.0 or args.pitch != 0.0):
        raise SystemExit("--aligned with --prosody / --energy / --voice scores tracks along the mels' warping path; with --speed / --pitch "
                         "the waveform is on another time axis: drop --aligned or the two flags")
    if args.rhythm is None and args.rhythm_window is not None:
        raise SystemExit("--rhythm_window acts on a plan: give --rhythm ref")
    from synthesizer import tempo_options
    tempo_options(args)                                                   # a value out of range is refused here
    return args


def read_rows(path, limit=None):
    """the rows (audio_path, text, speaker, emotion id) of a filelist, in order; the paths and labels through
    extract_latents.read_filelist, so both commands take the same files"""
    from extract_latents import read_filelist
    paths, emotions = read_filelist(path)
    rows = []
    with open(path, encoding='utf-8') as f:
        for line in f:
            if line.strip():
                _, text, speaker, _ = line.strip().split("|")
                rows.append((paths[len(rows)], text, speaker, int(emotions[len(rows)])))
    return rows if limit is None else rows[:limit]


def main(argv=None):
    args = parse_args(argv)
    from evaluation import summarize
    from hparams import create_hparams
    from synthesizer import GriffinLimVocoder, Synthesizer
    hp = create_hparams()
    hp.sampling_rate = 16000                 # the reference's Synthesizer() overrides, as synthesizer.py's command line
    hp.max_decoder_steps = 600
    if args.hparams:
        hp.parse(args.hparams)
    from synthesizer import tempo_options, weights_option
    from wavio import wav_options
    waveforms = args.prosody or args.energy or args.voice                 # the scores that need the vocoder
    syn = Synthesizer(hp, attention_window=args.attention_window, **tempo_options(args), **wav_options(args))
    if args.condition == 'emotion':
        syn.load(args.load_path, vocoder=args.vocoder if waveforms else None, filelist_path=args.filelist_path,
                 **weights_option(args))
    else:
        syn.load_checkpoint(args.load_path, **weights_option(args))
        if waveforms:
            syn.vocoder = GriffinLimVocoder.named(args.vocoder, syn.stft, syn.speed, syn.pitch_st, syn.formant, syn.preserve_formants)
    rows = read_rows(args.filelist_path, args.limit)
    style = dict(style=True, style_k=args.style_k) if args.style else {}
    timing = dict(durations=True, max_step=args.max_step) if args.durations else {}
    rhythm = dict(rhythm=args.rhythm, rhythm_window=args.rhythm_window) if args.rhythm else {}
    records = syn.evaluate(rows, args.batch_size, args.condition, prosody=args.prosody, alignment=args.alignment,
                           aligned=args.aligned, energy=args.energy, voice=args.voice, **style, **timing, **rhythm)
    summary = summarize(records)
    formant_keys = {}
    if args.formant != 0.0 or args.preserve_formants:                     # the report gains its new keys only with a new flag
        formant_keys = {'formant': syn.formant, 'preserve_formants': syn.preserve_formants}
    timing_keys = {'max_step': args.max_step} if args.durations else {}   # likewise
    if args.rhythm:
        timing_keys.update(rhythm=args.rhythm, rhythm_window=list(args.rhythm_window or Synthesizer.RHYTHM_WINDOW))
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump({'summary': summary, 'rows': [dict(r, path=row[0]) for r, row in zip(records, rows)],
                   'attention_window': None if syn.attention_window is None else list(syn.attention_window),
                   'weights': args.weights or 'raw', 'speed': syn.speed, 'pitch': syn.pitch_st, **formant_keys, **timing_keys},
                  f, indent=1)
    print(json.dumps(summary, indent=1))
    if args.alignment:
        for name, st in summary['by_emotion'].items():
            print("%s: dtw_mean %s, read_through_share %s (%d of %d rows that stopped)"
                  % (name, st['dtw_mean'], st['read_through_share'], st['n_read_through'], st['n_alignment']))
    if args.aligned:
        for name, st in summary['by_emotion'].items():
            print("%s: dtw_mean %s, mcd_db_mean %s, ffe_mean %s, warp_dev_mean %s (%d rows that stopped)"
                  % (name, st['dtw_mean'], st['mcd_db_mean'], st['ffe_mean'], st['warp_dev_mean'], st['n_aligned']))
    if args.durations:
        for name, st in summary['by_emotion'].items():
            print("%s: dtw_mean %s, dur_rmse_frames_mean %s, dur_corr_mean %s, dur_log_ratio_spread_mean %s, align_logp_rec_mean %s "
                  "(%d rows that stopped)" % (name, st['dtw_mean'], st['dur_rmse_frames_mean'], st['dur_corr_mean'],
                                              st['dur_log_ratio_spread_mean'], st['align_logp_rec_mean'], st['n_durations']))
    if args.energy:
        for name, st in summary['energy']['by_emotion'].items():
            print("%s: loudness_shift_lu_mean %s, loudness_vs_neu_lu %s (recordings %s), energy_spread_ratio_mean %s (%d rows)"
                  % (name, st['loudness_shift_lu_mean'], st['loudness_vs_neu_lu'], st['loudness_ref_vs_neu_lu'],
                     st['energy_spread_ratio_mean'], st['n_energy']))
    if args.voice:
        for name, st in summary['voice']['by_emotion'].items():
            print("%s: alpha_shift_db_mean %s, alpha_vs_neu_db %s (recordings %s), cpp_vs_neu_db %s (recordings %s) (%d rows)"
                  % (name, st['alpha_shift_db_mean'], st['alpha_vs_neu_db'], st['alpha_ref_vs_neu_db'], st['cpp_vs_neu_db'],
                     st['cpp_ref_vs_neu_db'], st['n_voice']))
    if args.style:
        st = summary['style']
        print("style: accuracy %s (recordings leave-one-out %s, k = %s), own recording nearest in %s of %d rows"
              % (st['overall']['accuracy'], st['ref_accuracy'], st['k'], st['overall']['rank0_share'], st['overall']['n_style']))
    print("%s: %d utterances" % (args.out, len(records)))


if __name__ == "__main__":
    main()
