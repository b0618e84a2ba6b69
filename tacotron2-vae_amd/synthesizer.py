"""Inference wrapper with the call sequence of the reference's `Synthesizer` (reference synthesizer.py:74-168,
README.md:157-253): load a checkpoint, build (or read) the per-emotion latent centroids, then synthesise a
mel from text conditioned either on a reference utterance or on an emotion-ratio mix.

Differences by design:
* the decode loop runs in the HIP inference session (`Decoder.inference`, 4 launches per frame) instead of
  Python-stepping `decode()`; the stepwise API is still there for callers that want it;
* the vocoder is pluggable: any callable mel(1,80,T) -> waveform, or `vocoder='griffin_lim'` / `'griffin_lim_fast'` for
  the built-in GriffinLimVocoder.  WaveGlow is an unpinned submodule of the reference and is out of scope here; without a vocoder
  `synthesize` writes the mel as `<path>.npy`.
"""
import os

import numpy as np
import torch

from hparams import create_hparams
from layers import TacotronSTFT
from text import text_to_sequence
from utils import load_wav_to_torch

EMOTIONS = ('neu', 'sad', 'ang', 'hap')      # label ids 0..3 of the koemo filelists


def length_groups(lengths, batch_size):
    """Indices of `lengths` sorted by length (longest first, ties in input order) and cut into groups of at most batch_size:
    the ragged batches of Synthesizer.latents, each padded only to its own longest item."""
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1, got %r" % (batch_size,))
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def wav_num_samples(path):
    """sample count of a wav from its header (the data is memory-mapped, not read)"""
    from scipy.io.wavfile import read
    return len(read(path, mmap=True)[1])


def resample_rows(items, target_rate):
    """items: [(sampling rate, 1-D numpy samples: int16 PCM or float32 in [-1, 1))], as `wavio.read_wav` gives them.  Returns
    (y (B, max count) float32 on the device, zero-padded, in the order of the items; counts at target_rate): the rows are
    grouped by (source rate, sample format), one upload and one `t2v_hip.resample` launch per group; a row's bits do not
    depend on its group."""
    import t2v_hip
    groups = {}
    for b, (rate, data) in enumerate(items):
        groups.setdefault((rate, data.dtype.str), []).append(b)
    parts, n = [], [0] * len(items)
    for (rate, _), idx in groups.items():
        counts = [len(items[b][1]) for b in idx]
        x = np.zeros((len(idx), max(counts)), dtype=items[idx[0]][1].dtype)
        for k, b in enumerate(idx):
            x[k, :counts[k]] = items[b][1]
        y_g, n_g = t2v_hip.resample(torch.from_numpy(x).cuda(), counts, rate, target_rate)
        parts.append((idx, y_g))
        for b, k in zip(idx, n_g):
            n[b] = k
    if len(parts) == 1:                                   # one group holds the items in their order
        return parts[0][1], n
    y = torch.zeros(len(items), max(n), device=parts[0][1].device)
    for idx, y_g in parts:
        y[torch.tensor(idx, device=y.device), :y_g.size(1)] = y_g
    return y, n


VOCODERS = ('griffin_lim', 'griffin_lim_fast', 'spsi')
# which weights of a checkpoint a Synthesizer loads -> the checkpoint key that holds them (train.save_checkpoint)
WEIGHTS = {'raw': 'state_dict', 'ema': 'ema_state_dict'}


def check_weights(weights):
    """None (= 'raw') or a name of WEIGHTS -> the name; ValueError otherwise"""
    if weights is None:
        return 'raw'
    if weights not in WEIGHTS:
        raise ValueError("weights must be one of %s or None, got %r" % (sorted(WEIGHTS), weights))
    return weights


class GriffinLimVocoder(object):
    """mel (B, 80, T) -> waveform (B, (T-1)*256) on the device: `stft.mel_to_magnitude` (pinv of the mel filterbank,
    clamped at 0) and n_iters Griffin-Lim iterations on `stft.stft_fn` (audio_processing.griffin_lim, initial phase from
    np.random).  The samples are not clipped: Griffin-Lim's output may exceed +-1 slightly.  Needs T >= 4 frames.
    momentum > 0: fast Griffin-Lim; inversion='nnls': the non-negative least-squares inverse of the filterbank
    (inversion_iters projected-gradient steps from the clamped pinv).  Neither changes which phases are drawn.
    speed (0.25..4, above 1 is faster) and pitch (semitones, -12..12), with p / q = 2^(pitch / 12) from `t2v_hip.pitch_ratio`:
    the linear magnitudes are stretched in time by speed q / p (`t2v_hip.stretch_magnitude`; Griffin-Lim makes the phases, so
    no phase vocoder is needed), Griffin-Lim runs on the stretched frames (at least 4 per row), and its waveform is resampled
    by p / q (`t2v_hip.resample`), which brings the duration back to 1 / speed and moves every frequency by p / q.  The
    initial phases are then drawn for the stretched frame counts.  speed=1, pitch=0 is the vocoder without them.
    formant (semitones, -12..12) moves the spectral envelope of the output up by 2^(formant / 12) and leaves the harmonics;
    preserve_formants keeps the envelope where it was under `pitch`, which alone moves it with the harmonics.  Both are one
    `t2v_hip.warp_envelope` of the linear magnitudes, before the stretch, by the ratio of `t2v_hip.vocoder_warp`;
    formant=0, preserve_formants=False is the vocoder without them.
    init='spsi': the initial phase is not drawn but computed on the device from the magnitudes Griffin-Lim sees, after the
    warp and the stretch (`t2v_hip.spsi_phase`, single-pass spectrogram inversion); np.random is not touched and no phase
    crosses from the host.  n_iters=0 then writes that start as it is, one inverse transform: `named('spsi')`, which keeps
    low voices voiced where the iterations lose them."""

    def __init__(self, stft, n_iters=60, momentum=0.0, inversion='pinv', inversion_iters=100, speed=1.0, pitch=0.0, formant=0.0,
                 preserve_formants=False, init='random'):
        from audio_processing import check_init
        from t2v_hip import check_momentum, vocoder_rates, vocoder_warp
        self.init = check_init(init)
        if inversion not in ('pinv', 'nnls'):
            raise ValueError("GriffinLimVocoder: inversion must be 'pinv' or 'nnls', got %r" % (inversion,))
        self.stft, self.n_iters = stft, n_iters
        self.momentum, self.inversion, self.inversion_iters = check_momentum(momentum), inversion, inversion_iters
        self.speed, self.pitch = float(speed), float(pitch)
        self.stretch, self.shift = vocoder_rates(speed, pitch)      # (num, den) of the magnitudes' rate, (p, q) of the pitch
        self.warp = vocoder_warp(pitch, formant, preserve_formants)  # (a, b): the envelope is read at k a / b
        self.formant, self.preserve_formants = float(formant), bool(preserve_formants)

    @classmethod
    def named(cls, name, stft, speed=1.0, pitch=0.0, formant=0.0, preserve_formants=False):
        """the vocoder behind load(vocoder=name) and the command lines' --vocoder"""
        knobs = dict(speed=speed, pitch=pitch, formant=formant, preserve_formants=preserve_formants)
        if name == 'griffin_lim':
            return cls(stft, **knobs)
        if name == 'griffin_lim_fast':
            return cls(stft, momentum=0.99, inversion='nnls', **knobs)
        if name == 'spsi':
            return cls(stft, n_iters=0, momentum=0.0, inversion='nnls', init='spsi', **knobs)
        raise ValueError("unknown vocoder %r (a callable, or one of %s)" % (name, ', '.join(repr(v) for v in VOCODERS)))

    def _magnitudes(self, mel, lengths):
        if self.inversion == 'pinv':
            return self.stft.mel_to_magnitude(mel, lengths)
        return self.stft.mel_to_magnitude(mel, lengths, self.inversion, self.inversion_iters)

    def _stretched(self, magnitudes, n):
        """the magnitudes with their envelope warped by self.warp, at the rate self.stretch, and their frame counts (as they
        came when neither is set)"""
        import t2v_hip
        if self.warp[0] != self.warp[1]:
            magnitudes = t2v_hip.warp_envelope(self.stft.stft_fn.on_gpu(magnitudes), n, self.warp)
        if self.stretch[0] == self.stretch[1]:
            return magnitudes, n
        for b, k in enumerate(n):
            if t2v_hip.stretch_frames(k, *self.stretch) < 4:
                raise ValueError("GriffinLimVocoder: row %d has %d frames, fewer than Griffin-Lim's 4 at the rate %d/%d"
                                 % (b, k, self.stretch[0], self.stretch[1]))
        return t2v_hip.stretch_magnitude(self.stft.stft_fn.on_gpu(magnitudes), n, self.stretch)

    def _shifted(self, wav, n):
        """Griffin-Lim's waveforms ((n[b] - 1) 256 samples each) resampled by p / q: (wav, sample counts)"""
        import t2v_hip
        counts = [(k - 1) * 256 for k in n]
        if self.shift[0] == self.shift[1]:
            return wav, counts
        return t2v_hip.resample(self.stft.stft_fn.on_gpu(wav), counts, *self.shift)

    def __call__(self, mel, lengths=None):
        from audio_processing import griffin_lim
        magnitudes = self._magnitudes(mel, lengths)
        if self.stretch[0] == self.stretch[1] and self.shift[0] == self.shift[1] and self.warp[0] == self.warp[1]:
            return griffin_lim(magnitudes, self.stft.stft_fn, self.n_iters, lengths=lengths, momentum=self.momentum, init=self.init)
        n = [magnitudes.size(2)] * magnitudes.size(0) if lengths is None else [int(x) for x in torch.as_tensor(lengths).reshape(-1).tolist()]
        stretched, n = self._stretched(magnitudes, n)
        wav = griffin_lim(stretched, self.stft.stft_fn, self.n_iters, lengths=n, momentum=self.momentum, init=self.init)
        return self._shifted(wav, n)[0].to(mel.device)

    def batch(self, mel, lengths):
        """A ragged batch in one set of launches, item by item as `self(mel[b:b+1, :, :lengths[b]])` would give it: the
        initial phases are drawn from np.random per item, in item order, with shape (1, 513, lengths[b]) — what B calls in
        a row draw.  With init='spsi' nothing is drawn and no phase array is built on the host: the start is a function of each
        row's magnitudes alone.  Returns a list of B waveforms ((lengths[b]-1)*256 samples each) on the device."""
        from audio_processing import griffin_lim
        n = [int(x) for x in torch.as_tensor(lengths).reshape(-1).tolist()]
        B = mel.size(0)
        magnitudes, n = self._stretched(self._magnitudes(mel, n), n)
        if self.init == 'spsi':
            wav = griffin_lim(magnitudes, self.stft.stft_fn, self.n_iters, lengths=n, momentum=self.momentum, init='spsi')
        else:
            angles = np.zeros((B, 513, magnitudes.size(2)), dtype=np.float32)
            for b, nb in enumerate(n):
                angles[b, :, :nb] = np.angle(np.exp(2j * np.pi * np.random.rand(1, 513, nb)))[0]
            wav = griffin_lim(magnitudes, self.stft.stft_fn, self.n_iters, angles=torch.from_numpy(angles), lengths=n,
                              momentum=self.momentum)
        wav, counts = self._shifted(wav, n)
        return [wav[b, :k] for b, k in enumerate(counts)]


class Synthesizer(object):
    def __init__(self, hparams=None, resample=False, trim_db=None, attention_window=None, speed=1.0, pitch=0.0, ref_speed=1.0,
                 ref_pitch=0.0, formant=0.0, ref_formant=0.0, preserve_formants=False):
        """speed, pitch: the tempo (0.25..4, above 1 is faster) and the pitch shift in semitones (-12..12) of what the built-in
        vocoder writes (`GriffinLimVocoder(speed=, pitch=)`, made in `load`): synthesize, synthesize_batch and the vocoder leg
        of evaluate pick them up through the vocoder object; ref_speed, ref_pitch: every reference wav that is read goes
        through `t2v_hip.time_stretch` / `t2v_hip.pitch_shift` before the mel front end ("say it like this clip, but faster /
        higher").  The reference knobs act where the wavs are read (`load_wavs`), so every consumer gets the perturbed clip:
        load_mel(s), latents, latent_map / latent_report, pitch, loudness, latent_probe (on top of its own perturbations) and
        both uses of the recordings in evaluate, the style and the `truth` mels; `wav_lengths`, which only sorts, still counts the
        files' samples.  All four are off by default.
        formant, ref_formant (semitones, -12..12) move the spectral envelope alone, the formants, and keep the harmonics: formant
        in the vocoder (`GriffinLimVocoder(formant=)`), ref_formant on every reference wav (`t2v_hip.formant_shift`, after the
        tempo and pitch steps).  preserve_formants makes both pitch knobs leave the envelope where it was: `pitch` through the
        vocoder's `preserve_formants`, `ref_pitch` through `t2v_hip.pitch_shift(preserve_formants=True)`; without it a pitch
        shift moves the formants with F0, which is another speaker ("like this clip, but higher" then wants it on).  All three
        are off by default.
        attention_window: None, or (back, ahead) for the decoder of every model this object loads (`Decoder.attention_window`:
        each free-running frame attends within [p - back, p + ahead] of the position p the previous frame attended most), so
        synthesize, synthesize_batch, alignment and evaluate all decode under it;
        resample: wavs at any sampling rate are resampled to hparams.sampling_rate on the device (`t2v_hip.resample`)
        instead of being refused; trim_db: leading and trailing silence is cut from every wav that is read
        (`t2v_hip.trim_bounds` at that many dB below the wav's loudest frame, 2 frames of margin, then `t2v_hip.crop`).
        Both are off by default, and both act in `load_wavs`, through which every method here reads its wavs."""
        if hparams is None:             # the reference's constructor (synthesizer.py:47-51): defaults + two overrides
            hparams = create_hparams()
            hparams.sampling_rate = 16000
            hparams.max_decoder_steps = 600
        self.hparams = hparams
        hp = self.hparams
        if trim_db is not None:
            trim_db = float(trim_db)
            if not 0.0 < trim_db < float('inf'):
                raise ValueError("trim_db must be a positive number of dB, got %r" % (trim_db,))
            if hp.hop_length != 256:
                raise ValueError("trim_db: the trim is built for hop 256, the front end has hop %d" % hp.hop_length)
        self.resample, self.trim_db = bool(resample), trim_db
        import t2v_hip
        t2v_hip.vocoder_rates(speed, pitch)                              # refused here, not at load()
        t2v_hip.vocoder_warp(pitch, formant, preserve_formants)
        self.speed, self.pitch_st = float(speed), float(pitch)         # `pitch` is the F0 tracker's method
        self.ref_speed, self.ref_pitch = float(ref_speed), float(ref_pitch)
        self.formant, self.ref_formant, self.preserve_formants = float(formant), float(ref_formant), bool(preserve_formants)
        self._ref_stretch, self._ref_shift = t2v_hip.stretch_ratio(ref_speed), t2v_hip.pitch_ratio(ref_pitch)
        self._ref_warp = t2v_hip.pitch_ratio(ref_formant)
        self._ref_perturbed = (self._ref_stretch[0] != self._ref_stretch[1] or self._ref_shift[0] != self._ref_shift[1]
                               or self._ref_warp[0] != self._ref_warp[1])
        from t2v_hip import check_attention_window
        self.attention_window = check_attention_window(attention_window)
        self.stft = TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_mel_channels,
                                 hp.sampling_rate, hp.mel_fmin, hp.mel_fmax)
        self.model = None
        self.weights = 'raw'         # the weight set of the loaded checkpoint (load_checkpoint(weights=))
        self.vocoder = None
        self.neu = self.sad = self.ang = self.hap = None

    # ------------------------------------------------------------------ audio -> mel (synthesizer.py:57-68)
    def load_mel(self, path):
        if self.resample or self.trim_db is not None or self._ref_perturbed:
            y, n = self.load_wavs([path])
            return self.stft.mel_spectrogram(y[:, :n[0]])
        audio, sampling_rate = load_wav_to_torch(path)
        if sampling_rate != self.hparams.sampling_rate:
            raise ValueError("{} SR doesn't match target {} SR".format(sampling_rate, self.hparams.sampling_rate))
        audio_norm = (audio / self.hparams.max_wav_value).unsqueeze(0)
        return self.stft.mel_spectrogram(audio_norm.cuda())

    def load_wavs(self, paths):
        """the wavs as one zero-padded batch on the device: (y (B, S_max) float32 in [-1, 1), sample counts); a wav whose rate
        is not hparams.sampling_rate is a ValueError, unless the Synthesizer was made with resample=True: then every wav is
        resampled to it on the device, one `t2v_hip.resample` launch per distinct source rate, and the counts are the
        resampled ones.  With trim_db the batch is trimmed and cropped before it is returned, and the counts are the trimmed
        ones."""
        if self.resample:
            y, n = self._load_wavs_any_rate(list(paths))
        else:
            y, n = self._load_wavs_at_rate(paths)
        if self.trim_db is not None:
            import t2v_hip
            from wavio import DEFAULT_PAD_FRAMES
            y, n = t2v_hip.crop(y, t2v_hip.trim_bounds(y, n, self.trim_db, DEFAULT_PAD_FRAMES))
        return y, n

    def _load_wavs_any_rate(self, paths):
        from wavio import read_wav
        if not paths:
            raise ValueError("load_wavs: no paths")
        return self._perturb_refs(*resample_rows([read_wav(path) for path in paths], self.hparams.sampling_rate))

    def _perturb_refs(self, y, n):
        """ref_speed, ref_pitch and ref_formant on a batch of wavs that has just been read (as it came when all are off)"""
        if not self._ref_perturbed:
            return y, n
        import t2v_hip
        y, n = t2v_hip.time_stretch(y, n, self._ref_stretch)
        y, n = t2v_hip.pitch_shift(y, n, self.ref_pitch, preserve_formants=self.preserve_formants)
        return t2v_hip.formant_shift(y, n, self.ref_formant)

    def _load_wavs_at_rate(self, paths):
        audios = []
        for path in paths:
            audio, sampling_rate = load_wav_to_torch(path)
            if sampling_rate != self.hparams.sampling_rate:
                raise ValueError("{} SR doesn't match target {} SR".format(sampling_rate, self.hparams.sampling_rate))
            audios.append(audio / self.hparams.max_wav_value)
        if not audios:
            raise ValueError("load_wavs: no paths")
        n = [a.numel() for a in audios]
        y = torch.zeros(len(audios), max(n))
        for b, a in enumerate(audios):
            y[b, :n[b]] = a
        return self._perturb_refs(y.cuda(), n)

    def wav_lengths(self, paths):
        """sample counts of the wavs as `load_wavs` will count them before any trim (and before ref_speed / ref_pitch, which
        change them by the rate), from their headers: the file's count, or
        with resample=True ceil(count up / down) at the front end's rate; what the length sorting of `latents` and `pitch`
        goes by"""
        if not self.resample:
            return [wav_num_samples(p) for p in paths]
        import t2v_hip
        from wavio import wav_header
        out = []
        for p in paths:
            rate, count, _ = wav_header(p)
            out.append(t2v_hip.resample_length(count, *t2v_hip.resample_ratio(rate, self.hparams.sampling_rate)))
        return out

    def _mels_of(self, y, n):
        mels = self.stft.mel_spectrogram(y, torch.tensor(n, dtype=torch.int64))
        return mels, [k // self.hparams.hop_length + 1 for k in n]

    def load_mels(self, paths):
        """`load_mel` for several wavs in one ragged front-end call: returns (mels (B, 80, T_max) on the device, frame counts);
        item b equals load_mel(paths[b]) on its first counts[b] frames, and what lies past them is padding."""
        paths = list(paths)
        if not paths:
            raise ValueError("load_mels: no paths")
        return self._mels_of(*self.load_wavs(paths))

    def _wav_groups(self, who, paths, batch_size):
        """the loop of pitch, loudness, voice_quality, latents and latent_probe: an empty list is refused in who's name; the
        wavs are sorted by length (`wav_lengths`) and read (`load_wavs`) in ragged batches of at most batch_size; yields
        (indices into paths, y, sample counts) per batch"""
        if not paths:
            raise ValueError("%s: no paths" % who)
        for idx in length_groups(self.wav_lengths(paths), batch_size):
            y, n = self.load_wavs([paths[i] for i in idx])
            yield idx, y, n

    # the refusals that pitch, loudness, voice_quality and evaluate share; `who` opens the message
    def _need_griffin_lim(self, who):
        if not isinstance(self.vocoder, GriffinLimVocoder):
            raise RuntimeError("%s needs the Griffin-Lim vocoder: load(..., vocoder='griffin_lim')" % who)

    def _need_tracker_grid(self, who):
        import t2v_hip
        if self.hparams.sampling_rate != t2v_hip.F0_SAMPLE_RATE or self.hparams.hop_length != t2v_hip.F0_HOP:
            raise ValueError("%s: the tracker is built for %d Hz and hop %d, the front end has %d Hz and hop %d"
                             % (who, t2v_hip.F0_SAMPLE_RATE, t2v_hip.F0_HOP, self.hparams.sampling_rate, self.hparams.hop_length))

    def _need_frame_grid(self, who):
        import t2v_hip
        if self.hparams.hop_length != t2v_hip.TRIM_HOP:
            raise ValueError("%s: the frame track is built for hop %d, the front end has hop %d"
                             % (who, t2v_hip.TRIM_HOP, self.hparams.hop_length))

    @torch.no_grad()
    def pitch(self, paths, batch_size=64):
        """F0 tracks of the wavs (`t2v_hip.f0`: YIN on the front end's frames, Hz, 0 where unvoiced), in input order: a list
        of 1-D device tensors, paths[i]'s of its own samples // 256 + 1 frames, each what f0 gives for that wav alone.  The
        wavs are sorted by length and run in ragged batches of at most batch_size."""
        import t2v_hip
        paths = list(paths)
        self._need_tracker_grid('pitch')
        tracks = [None] * len(paths)
        for idx, y, n in self._wav_groups('pitch', paths, batch_size):
            hz = t2v_hip.f0(y, n)
            for b, i in enumerate(idx):
                tracks[i] = hz[b, :n[b] // t2v_hip.F0_HOP + 1]
        return tracks

    @torch.no_grad()
    def loudness(self, paths, batch_size=64):
        """Loudness and energy of the wavs (`t2v_hip.loudness`: ITU-R BS.1770-4, K-weighted and gated), in input order: one
        dict per wav with `loudness_lufs` (integrated; -inf for a wav without a gated 400 ms block), `momentary_max_lufs` (its
        loudest block) and `energy_db` (1-D device tensor: the K-weighted level of the front end's samples // 256 + 1 frames,
        `t2v_hip.energy_db`), each what the meter gives for that wav alone.  The wavs go through `load_wavs` (resample= and
        trim_db= apply), sorted by length, in ragged batches of at most batch_size."""
        import t2v_hip
        paths = list(paths)
        self._need_frame_grid('loudness')
        out = [None] * len(paths)
        for idx, y, n in self._wav_groups('loudness', paths, batch_size):
            r = t2v_hip.loudness(y, n, self.hparams.sampling_rate)
            db = t2v_hip.energy_db(r.frame_ms)
            for b, i in enumerate(idx):
                out[i] = {'loudness_lufs': r.integrated[b], 'momentary_max_lufs': r.momentary_max[b],
                          'energy_db': db[b, :n[b] // t2v_hip.TRIM_HOP + 1]}
        return out

    def _need_voice_grid(self, who):
        """the voice-quality bands are bins of the front end's frames at 16 kHz"""
        import t2v_hip
        self._need_frame_grid(who)
        if self.hparams.sampling_rate != t2v_hip.F0_SAMPLE_RATE:
            raise ValueError("%s: the voice-quality bands are laid out for %d Hz, the front end has %d Hz"
                             % (who, t2v_hip.F0_SAMPLE_RATE, self.hparams.sampling_rate))

    @torch.no_grad()
    def voice_quality(self, paths, batch_size=64):
        """Voice quality of the wavs (`t2v_hip.voice_quality`: spectral balance and cepstral peak prominence per frame), in
        input order: one dict per wav with the six tracks of `t2v_hip.VOICE_FEATS` by name, 1-D device tensors of the front
        end's samples // 256 + 1 frames, each what the kernel gives for that wav alone.  The wavs go through `load_wavs`
        (resample= and trim_db= apply), sorted by length, in ragged batches of at most batch_size."""
        import t2v_hip
        paths = list(paths)
        self._need_voice_grid('voice_quality')
        out = [None] * len(paths)
        for idx, y, n in self._wav_groups('voice_quality', paths, batch_size):
            vq = t2v_hip.voice_quality(y, n)
            for b, i in enumerate(idx):
                out[i] = {k: getattr(vq, k)[b, :n[b] // t2v_hip.TRIM_HOP + 1] for k in t2v_hip.VOICE_FEATS}
        return out

    @torch.no_grad()
    def latents(self, paths, batch_size=64):
        """(prosody (N, E), mu, logvar, z (N, z_latent_dim)) of every wav, in input order, each row what
        `model.vae_gst(load_mel(paths[i]))` returns (up to fp32 summation order).  The wavs are sorted by length and run in
        ragged batches of at most batch_size (one front-end call and one vae_gst call each)."""
        paths = list(paths)
        parts, order = [], []
        for idx, y, n in self._wav_groups('latents', paths, batch_size):
            parts.append(self.model.vae_gst(*self._mels_of(y, n)))
            order += idx
        inv = torch.empty(len(paths), dtype=torch.int64)
        inv[torch.tensor(order)] = torch.arange(len(paths))
        inv = inv.to(parts[0][0].device)
        return tuple(torch.cat([p[k] for p in parts], 0)[inv] for k in range(4))

    def latent_map(self, paths, key='mus', batch_size=64, **tsne_kwargs):
        """(N, 2) exact t-SNE map of the wavs' latents: `latents(paths)` followed by `t2v_hip.tsne` on prosody, mus, logvars
        or zs (key); tsne_kwargs (perplexity, n_iter, seed, init, return_trace) go to `t2v_hip.tsne` as they are."""
        import t2v_hip
        keys = ('prosody', 'mus', 'logvars', 'zs')
        if key not in keys:
            raise ValueError("key must be one of %s, got %r" % (', '.join(keys), key))
        return t2v_hip.tsne(self.latents(paths, batch_size)[keys.index(key)].float().contiguous(), **tsne_kwargs)

    def latent_report(self, paths, emotions, key='mus', k=5, batch_size=64):
        """Does the latent separate the emotions?  `latents(paths)` followed by `latent_scores.corpus_report` on mus or zs
        (key) with the label ids `emotions`: leave-one-out kNN accuracy and confusion matrix, silhouette, active units and KL
        per dimension (those two always from mus and logvars), as one JSON-serialisable dict."""
        from latent_scores import corpus_report
        keys = {'mus': 1, 'zs': 3}
        if key not in keys:
            raise ValueError("key must be one of mus, zs, got %r" % (key,))
        paths, emotions = list(paths), [int(e) for e in emotions]
        if len(paths) != len(emotions):
            raise ValueError("latent_report: %d paths for %d emotion labels" % (len(paths), len(emotions)))
        lat = [t.float().cpu().numpy() for t in self.latents(paths, batch_size)]
        return corpus_report(lat[keys[key]], emotions, lat[1], lat[2], k)

    @torch.no_grad()
    def latent_probe(self, paths, emotions=None, pitch=(-2, 2), speed=(0.85, 1.15), gain_db=(-6, 6), batch_size=64, formant=(),
                     preserve_formants=False):
        """What does the latent listen to?  Every wav is encoded as it is and under each single perturbation: a pitch shift
        (semitones, `t2v_hip.pitch_shift`), a tempo change (`t2v_hip.time_stretch`) or a gain (dB, `t2v_hip.scale_rows`), applied
        to the samples `load_wavs` gives, before the mel front end.  Returns a JSON-serialisable dict: `n_clips`, `scale`,
        `scale_kind` and `perturbations`, one entry per value in the order pitch, speed, gain_db with `kind`, `value`, the
        `mean` and `median` over the clips of ||mu' - mu||_2, and `mean_rel` / `median_rel`, those divided by `scale`.
        scale: the mean distance between the emotions' centroids of mu when emotions (one label id per path) are given and
        hold two labels or more (`scale_kind` 'emotion_centroids'), else the mean distance between different clips' mu
        ('clip_pairs'); None, and None on the relative values, when there is no pair or the scale is 0.  There are no
        thresholds.  The wavs are sorted by length and run in ragged batches of at most batch_size; a clip and its
        perturbed copies are encoded in batches of the same rows, so the identity perturbation gives exactly 0.
        The plain pitch shift moves the formants with F0, two correlates at once.  preserve_formants=True makes the 'pitch'
        entries `t2v_hip.pitch_shift(preserve_formants=True)`, F0 alone, and formant=(semitones, ...) adds entries of kind
        'formant' after gain_db, `t2v_hip.formant_shift`: the envelope alone.  Together they tell whether mu listens to pitch
        or to timbre."""
        import t2v_hip
        paths = list(paths)
        if not paths:
            raise ValueError("latent_probe: no paths")
        if self.model is None:
            raise RuntimeError("latent_probe: no model (load_checkpoint() or load() first)")
        if emotions is not None:
            emotions = [int(e) for e in emotions]
            if len(emotions) != len(paths):
                raise ValueError("latent_probe: %d paths for %d emotion labels" % (len(paths), len(emotions)))
        probes = [('pitch', float(v)) for v in pitch] + [('speed', float(v)) for v in speed] + [('gain_db', float(v)) for v in gain_db]
        probes += [('formant', float(v)) for v in formant]
        for kind, v in probes:                                            # refused before any work
            if kind in ('pitch', 'formant'):
                t2v_hip.pitch_ratio(v)
            elif kind == 'speed':
                t2v_hip.stretch_ratio(v)
        N = len(paths)
        base = [None] * N
        dist = [[0.0] * N for _ in probes]
        for idx, y, n in self._wav_groups('latent_probe', paths, batch_size):
            mu = self.model.vae_gst(*self._mels_of(y, n))[1].double()
            for b, i in enumerate(idx):
                base[i] = mu[b].cpu().numpy()
            for k, (kind, v) in enumerate(probes):
                if kind == 'pitch':
                    y2, n2 = t2v_hip.pitch_shift(y, n, v, preserve_formants=bool(preserve_formants))
                elif kind == 'formant':
                    y2, n2 = t2v_hip.formant_shift(y, n, v)
                elif kind == 'speed':
                    y2, n2 = t2v_hip.time_stretch(y, n, v)
                else:
                    y2, n2 = t2v_hip.scale_rows(y.clone(), n, [10.0 ** (v / 20.0)] * len(idx)), n
                mu2 = self.model.vae_gst(*self._mels_of(y2, n2))[1].double()
                d = (mu2 - mu).pow(2).sum(1).sqrt().cpu().tolist()
                for b, i in enumerate(idx):
                    dist[k][i] = d[b]
        base = np.stack(base)

        def mean_pair_distance(x):
            if len(x) < 2:
                return None
            d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
            return float(d[np.triu_indices(len(x), 1)].mean())

        scale, kind = None, 'clip_pairs'
        if emotions is not None and len(set(emotions)) >= 2:
            lab = np.asarray(emotions)
            scale, kind = mean_pair_distance(np.stack([base[lab == c].mean(0) for c in sorted(set(emotions))])), 'emotion_centroids'
        else:
            scale = mean_pair_distance(base)
        if scale is not None and not scale > 0.0:
            scale = None
        out = []
        for (pk, v), d in zip(probes, dist):
            mean, median = float(np.mean(d)), float(np.median(d))
            out.append({'kind': pk, 'value': v, 'mean': mean, 'median': median,
                        'mean_rel': mean / scale if scale else None, 'median_rel': median / scale if scale else None})
        return {'n_clips': N, 'scale': scale, 'scale_kind': kind, 'perturbations': out}

    # ------------------------------------------------------------------ checkpoint + centroids (synthesizer.py:74-110)
    @staticmethod
    def centroid_cache_path(checkpoint_path, filelist_path, weights=None):
        """`<dir of ckpt>/<ckpt name>_<last '_' field of the filelist name, sans extension>.npz`; the averaged weights have
        latents of their own, hence a cache of their own: `<ckpt name>_ema_<...>.npz` with weights='ema'"""
        suffix = filelist_path.rsplit('_', 1)[1].split('.')[0] if '_' in filelist_path else 'refs'
        if check_weights(weights) == 'ema':
            suffix = 'ema_' + suffix
        return os.path.join(os.path.dirname(checkpoint_path), os.path.basename(checkpoint_path) + '_' + suffix + '.npz')

    def load_checkpoint(self, checkpoint_path, weights=None):
        """the model of a train.py checkpoint, in eval mode (the first step of `load`).  weights: None or 'raw' = the
        checkpoint's 'state_dict'; 'ema' = its 'ema_state_dict', the averaged weights a run with hparams.ema_decay > 0 saves
        (ValueError when the checkpoint has none)."""
        from train import load_model
        key = WEIGHTS[check_weights(weights)]
        ckpt = torch.load(checkpoint_path, map_location='cpu')
        if key not in ckpt:
            raise ValueError("checkpoint %r holds no %r (weights=%r needs a run with hparams.ema_decay > 0)"
                             % (checkpoint_path, key, weights))
        self.model = load_model(self.hparams)
        self.model.load_state_dict(ckpt[key])
        self.model.eval()
        self.model.decoder.attention_window = self.attention_window
        self.weights = check_weights(weights)
        return self

    def load(self, checkpoint_path, waveglow_path=None, vocoder=None,
             filelist_path='./web/static/uploads/koemo_spk_emo_all_test.txt', batch_size=64, weights=None):
        """Positional order of the reference (synthesizer.py:74: `load(checkpoint_path, waveglow_path)`, called from
        app.py:161).  waveglow_path: a WaveGlow checkpoint `{'model': module}` exactly as the reference loads it
        (needs the `waveglow` package importable: it is an un-vendored submodule of the reference); `vocoder`: any
        callable mel (1,80,T) -> audio instead, or 'griffin_lim' for GriffinLimVocoder(self.stft), or 'griffin_lim_fast' for
        the same with momentum 0.99 and the non-negative least-squares mel inversion, or 'spsi' for that inversion, a phase made
        from the magnitudes' peaks and no iteration (GriffinLimVocoder.named).  A callable passed in the second
        position is taken as the vocoder.  batch_size: wavs per ragged vae_gst call of the centroid pass
        (`latents`), when there is no centroid cache yet.  weights: see load_checkpoint (the centroid cache of the averaged
        weights is a file of its own)."""
        check_weights(weights)
        if isinstance(vocoder, str):
            # an unknown name fails before anything is loaded
            vocoder = GriffinLimVocoder.named(vocoder, self.stft, self.speed, self.pitch_st, self.formant, self.preserve_formants)
        self.load_checkpoint(checkpoint_path, weights=weights)
        if callable(waveglow_path) and vocoder is None:
            vocoder, waveglow_path = waveglow_path, None
        self.waveglow = None
        if waveglow_path is not None:
            try:
                self.waveglow = torch.load(waveglow_path, map_location='cpu', weights_only=False)['model'].cuda()
            except Exception as e:
                raise RuntimeError("cannot load the WaveGlow checkpoint %r (the reference's vocoder is an un-vendored "
                                   "submodule; its package must be importable): %s" % (waveglow_path, e))
            if vocoder is None:
                waveglow = self.waveglow
                vocoder = lambda mel: waveglow.infer(mel, sigma=0.666)      # reference synthesizer.py:163
        self.vocoder = vocoder
        npz_path = self.centroid_cache_path(checkpoint_path, filelist_path, weights)
        if os.path.exists(npz_path):
            d = np.load(npz_path)
            zs, emotions = d['zs'], d['emotions']
        else:
            with open(filelist_path, encoding='utf-8') as f:
                rows = [line.strip().split("|") for line in f if line.strip()]
            paths, emotions = [], []
            for audio_path, _, _, emotion in rows:
                paths.append(audio_path)
                emotions.append(int(emotion))
            emotions = np.array(emotions)
            zs = self.latents(paths, batch_size)[3].cpu().numpy()          # filelist order
            np.savez(npz_path, zs=zs, emotions=emotions)
        for i, name in enumerate(EMOTIONS):
            sel = zs[emotions == i, :]
            setattr(self, name, np.mean(sel, axis=0) if len(sel) else np.zeros(zs.shape[1], dtype=zs.dtype))
        return self

    # ------------------------------------------------------------------ text -> mel (synthesizer.py:112-168)
    def encode_text(self, text):
        sequence = np.array(text_to_sequence(text, ['korean_cleaners']))[None, :]
        sequence = torch.from_numpy(sequence).cuda().long()
        inputs = self.model.parse_input(sequence)
        embedded = self.model.transcript_embedding(inputs).transpose(1, 2)
        return self.model.encoder.inference(embedded)

    def style_vector(self, transcript_outputs, condition_on_ref, ref_audio, ratios):
        if condition_on_ref:
            latent, _, _, _ = self.model.vae_gst(self.load_mel(ref_audio))
            return latent.unsqueeze(1).expand_as(transcript_outputs)
        # ratio order of the reference: (neu, sad, hap, ang) — synthesizer.py:129-130
        mix = ratios[0] * self.neu + ratios[1] * self.sad + ratios[2] * self.hap + ratios[3] * self.ang
        return self.model.vae_gst.fc3(torch.as_tensor(mix, dtype=torch.float32).cuda())

    RHYTHM_WINDOW = (1, 1)      # the window around a planned symbol; uncalibrated: no trained checkpoint has been decoded under a plan

    def rhythm_plan(self, texts, lens, durations=None, rhythm_from=None, rhythm_scale=1.0, rhythm_window=None):
        """The decoder's plan keywords for `texts` (lens: their symbol counts), or {} when neither durations nor rhythm_from is
        given.  durations: per text n_symbols numbers, frames per symbol (fractions allowed); rhythm_from: per text a wav that
        speaks the same text, whose symbol durations `self.durations` measures (a wav on which the search finds no path is a
        ValueError naming it); rhythm_scale: a number, or per text n_symbols factors, multiplied in; rhythm_window: the
        (back, ahead) the decoder may look around the planned symbol (default RHYTHM_WINDOW; (0, 0) reads exactly one symbol per
        frame).  The plan is made by `t2v_hip.duration_plan` and cut at the decoder's max_decoder_steps; a text that gets no
        frame at all is a ValueError."""
        import t2v_hip
        B = len(texts)
        if durations is None and rhythm_from is None:
            if rhythm_window is not None or not (np.isscalar(rhythm_scale) and float(rhythm_scale) == 1.0):
                raise ValueError("rhythm_scale and rhythm_window act on a plan: give durations or rhythm_from")
            return {}
        if durations is not None and rhythm_from is not None:
            raise ValueError("give durations or rhythm_from, not both")
        if rhythm_from is not None:
            if len(rhythm_from) != B:
                raise ValueError("rhythm_from: %d wavs for %d texts" % (len(rhythm_from), B))
            found = self.durations([(w, t, None, 0) for w, t in zip(rhythm_from, texts)])
            for b, r in enumerate(found):
                if r['durations'] is None:
                    raise ValueError("rhythm_from: text %d has %d symbols and %s only %d frames: no monotonic path reads it"
                                     % (b, r['n_symbols'], rhythm_from[b], r['n_frames']))
            durations = [r['durations'] for r in found]
        if len(durations) != B:
            raise ValueError("durations: %d rows for %d texts" % (len(durations), B))
        dur = np.zeros((B, max(lens)), dtype=np.float32)
        for b, d in enumerate(durations):
            d = np.asarray(d, dtype=np.float32).reshape(-1)
            if d.size != lens[b]:
                raise ValueError("durations: text %d has %d symbols, got %d durations" % (b, lens[b], d.size))
            dur[b, :lens[b]] = d
        if np.isscalar(rhythm_scale):
            rate = float(rhythm_scale)
        else:
            if len(rhythm_scale) != B:
                raise ValueError("rhythm_scale: %d rows for %d texts" % (len(rhythm_scale), B))
            r = np.ones((B, max(lens)), dtype=np.float32)
            for b, f in enumerate(rhythm_scale):
                f = np.asarray(f, dtype=np.float32).reshape(-1)
                if f.size != lens[b]:
                    raise ValueError("rhythm_scale: text %d has %d symbols, got %d factors" % (b, lens[b], f.size))
                r[b, :lens[b]] = f
            rate = torch.from_numpy(r).cuda()
        out = t2v_hip.duration_plan(torch.from_numpy(dur).cuda(), lens, self.model.decoder.max_decoder_steps, rate=rate)
        for b, n in enumerate(out.n_plan.tolist()):
            if n < 1:
                raise ValueError("durations: text %d gets no frame" % b)
        return dict(plan=out.plan, n_plan=out.n_plan, plan_stop='plan',
                    plan_window=self.RHYTHM_WINDOW if rhythm_window is None else rhythm_window)

    @torch.no_grad()
    def synthesize(self, text, path=None, condition_on_ref=False, ref_audio=None, ratios=(1.0, 0.0, 0.0, 0.0), durations=None,
                   rhythm_from=None, rhythm_scale=1.0, rhythm_window=None):
        """Returns (mel_outputs_postnet (1,80,T), alignments (1,T,T_in)); writes `path` (wav through the vocoder,
        else `<path>.npy`) when a path is given.
        durations (n_symbols numbers), rhythm_from (a wav speaking the same text), rhythm_scale (a number or n_symbols factors),
        rhythm_window: the rhythm of `rhythm_plan`, for this one text; the output then has the plan's frame count.  The style
        stays what condition_on_ref / ratios say."""
        transcript_outputs = self.encode_text(text)
        encoder_outputs = transcript_outputs + self.style_vector(transcript_outputs, condition_on_ref, ref_audio, ratios)
        plan = self.rhythm_plan([text], [transcript_outputs.size(1)], None if durations is None else [durations],
                                None if rhythm_from is None else [rhythm_from],
                                rhythm_scale if np.isscalar(rhythm_scale) else [rhythm_scale], rhythm_window)
        mel_outputs, gate_outputs, alignments = self.model.decoder.inference(encoder_outputs, **plan)
        mel_outputs_postnet = mel_outputs + self.model.postnet(mel_outputs)
        if path is not None:
            if self.vocoder is not None:
                self._write_wav(path, self.vocoder(mel_outputs))
            else:
                np.save(path + '.npy', mel_outputs_postnet[0].detach().cpu().numpy())
        return mel_outputs_postnet, alignments

    def _write_wav(self, path, audio):
        from scipy.io.wavfile import write
        audio = audio[0] if torch.is_tensor(audio) and audio.dim() > 1 else audio
        write(path, self.hparams.sampling_rate, np.asarray(torch.as_tensor(audio).detach().cpu().float()))

    def _synthesize_ragged(self, texts, condition_on_ref, ref_audios, ratios, ref_mels=None, rhythm=None):
        """The device part of synthesize_batch: (mel, mel_postnet (B,80,N), gate (B,N,1), alignments, n_frames (B,) int64 on
        the host, text lengths).  ref_mels: `load_mels(list(dict.fromkeys(ref_audios)))` when the caller has it already.
        rhythm: None, or the keywords of `rhythm_plan` behind (texts, lens)."""
        B = len(texts)
        if condition_on_ref and (ref_audios is None or len(ref_audios) != B):
            raise ValueError("condition_on_ref needs one reference audio per text")
        if len(ratios) and not np.isscalar(ratios[0]):
            if len(ratios) != B:
                raise ValueError("ratios: %d tuples for %d texts" % (len(ratios), B))
            per_text = list(ratios)
        else:
            per_text = [ratios] * B
        seqs = [text_to_sequence(t, ['korean_cleaners']) for t in texts]
        lens = [len(q) for q in seqs]
        if min(lens) < 1:
            raise ValueError("a text maps to no symbols")
        ids = np.zeros((B, max(lens)), dtype=np.int64)        # pad id 0: masked out by the encoder, never read
        for b, q in enumerate(seqs):
            ids[b, :len(q)] = q
        ids = torch.from_numpy(ids).cuda()
        lengths = torch.tensor(lens, dtype=torch.int32).cuda()
        embedded = self.model.transcript_embedding(self.model.parse_input(ids)).transpose(1, 2)
        transcript_outputs = self.model.encoder.inference(embedded, lengths)              # (B, L, 512), 0 past each length
        if condition_on_ref:        # every distinct reference wav once, all in one ragged front-end + vae_gst call
            uniq = list(dict.fromkeys(ref_audios))
            mels, n = self.load_mels(uniq) if ref_mels is None else ref_mels
            latent = self.model.vae_gst(mels, n)[0]
            styles = [latent[uniq.index(p)].view(1, 1, -1) for p in ref_audios]
        else:
            styles = [self.style_vector(transcript_outputs[b:b + 1, :lens[b]], False, None, per_text[b]) for b in range(B)]
        encoder_outputs = torch.cat([transcript_outputs[b:b + 1] + styles[b].reshape(1, -1, styles[b].size(-1))[:, :1]
                                     for b in range(B)], 0)
        plan = self.rhythm_plan(texts, lens, **rhythm) if rhythm else {}
        mel, gate, alignments, n_frames = self.model.decoder.inference_batch(encoder_outputs, lens, **plan)
        mel_postnet = mel + self.model.postnet(mel, n_frames.to(torch.int32).cuda())
        return mel, mel_postnet, gate, alignments, n_frames, lens

    @torch.no_grad()
    def synthesize_batch(self, texts, paths=None, condition_on_ref=False, ref_audios=None, ratios=(1.0, 0.0, 0.0, 0.0),
                         durations=None, rhythm_from=None, rhythm_scale=1.0, rhythm_window=None):
        """`synthesize` for several texts at once: returns the list of what `synthesize(texts[i], paths[i], ...)` called
        for i = 0, 1, ... in turn would return from the same model state — frame counts, mels, alignments and Prenet dropout
        masks (the decoder reserves the seeds of len(texts) consecutive inference() calls), and, with the Griffin-Lim
        vocoder and the same np.random state, the same waveforms.  The texts run through the encoder, the decoder (groups
        of <= 8, sorted by length) and the Postnet as one ragged batch; each is masked to its own length.
        ratios: one (neu, sad, hap, ang) tuple for all texts, or one per text; ref_audios: one path per text
        (condition_on_ref); paths: None or one output path per text (wav through the vocoder, else `<path>.npy`).
        durations, rhythm_from (one entry per text), rhythm_scale, rhythm_window: the rhythm of `rhythm_plan`.  Text i then
        has the frames of its plan and reads symbol j over the frames the plan gives it."""
        B = len(texts)
        if B == 0:
            return []
        if paths is not None and len(paths) != B:
            raise ValueError("paths: %d paths for %d texts" % (len(paths), B))
        rhythm = dict(durations=durations, rhythm_from=rhythm_from, rhythm_scale=rhythm_scale, rhythm_window=rhythm_window)
        if durations is None and rhythm_from is None:
            self.rhythm_plan(texts, [], **rhythm)          # (refuses a scale or a window without a plan)
            rhythm = None
        mel, mel_postnet, _, alignments, n_frames, lens = self._synthesize_ragged(texts, condition_on_ref, ref_audios, ratios,
                                                                                  rhythm=rhythm)
        n = n_frames.tolist()
        out = [(mel_postnet[b:b + 1, :, :n[b]], alignments[b:b + 1, :n[b], :lens[b]]) for b in range(B)]
        if paths is not None:
            if self.vocoder is None:
                for b in range(B):
                    np.save(paths[b] + '.npy', out[b][0][0].detach().cpu().numpy())
            elif isinstance(self.vocoder, GriffinLimVocoder):
                for b, audio in enumerate(self.vocoder.batch(mel, n)):
                    self._write_wav(paths[b], audio)
            else:
                for b in range(B):
                    self._write_wav(paths[b], self.vocoder(mel[b:b + 1, :, :n[b]]))
        return out

    @staticmethod
    def _alignment_rows(al, n, lens, with_path=False):
        """(one dict of evaluation.ALIGNMENT_KEYS per row, the host paths or None) of a group's alignments (B, N, T_in), frame
        counts and text lengths: one `t2v_hip.alignment_stats` call and one copy to the host (focus rides along as an int32
        bit pattern next to the stats, and the paths when asked for)"""
        import t2v_hip
        from evaluation import alignment_fields
        r = t2v_hip.alignment_stats(al, n, lens)
        parts = [r.stats, r.focus.view(torch.int32)[:, None]] + ([r.path] if with_path else [])
        host = torch.cat(parts, 1).cpu()
        focus = host[:, 8].contiguous().view(torch.float32).tolist()
        stats = host[:, :8].tolist()
        fields = [alignment_fields(focus[b], stats[b], n[b], lens[b]) for b in range(len(n))]
        return fields, (host[:, 9:] if with_path else None)

    def _forced_alignments(self, texts, mels, n_frames, which=None):
        """The teacher-forced alignments of recordings against texts: row b is texts[b] read against the first
        n_frames[which[b]] frames of mels[which[b]] (which: None = row b's own).  One model forward per row, B = 1: the
        reference's encoder convolutions see the pad embedding of a padded batch, so only a batch of one gives the utterance
        alone.  eval mode, no gradients; the Prenet dropout stays on as in the reference (model.Prenet), with the masks of
        hparams.seed at the teacher-forced mask index of a model's first forward: the conv-block counter that index is taken
        from is set to 0 for every row and put back afterwards, and so is the decoder's call counter, so a row's alignment
        depends on nothing that ran before it and the free-running seeds go on as if this had not run.  Returns a list of
        (n_frames, n_symbols) device tensors."""
        import model as M
        self.model.eval()
        dec = self.model.decoder
        calls, blocks = dec._calls, M._block_calls[0]
        out = []
        try:
            with torch.no_grad():
                for b, text in enumerate(texts):
                    k = b if which is None else which[b]
                    ids = text_to_sequence(text, ['korean_cleaners'])
                    if len(ids) < 1:
                        raise ValueError("a text maps to no symbols")
                    M._block_calls[0] = 0
                    dev = mels.device
                    inputs = (torch.tensor([ids], dtype=torch.int64, device=dev), torch.tensor([len(ids)], dtype=torch.int64, device=dev),
                              mels[k:k + 1, :, :n_frames[k]].contiguous(), len(ids),
                              torch.tensor([n_frames[k]], dtype=torch.int64, device=dev), None, None)
                    out.append(self.model(inputs)[3][0, :n_frames[k], :len(ids)])      # cut to the true frame count
        finally:
            dec._calls, M._block_calls[0] = calls, blocks
        return out

    @staticmethod
    def _search_rows(als, max_step):
        """`t2v_hip.mas` on a list of (frames, symbols) device tensors: they are copied into one zero-padded tensor and searched
        in one call; a row without a feasible path is left out of it.  Returns (per row None or (durations, starts: host lists of
        its symbols, mean log-probability), durations, starts: (rows, widest symbols) int32 on the device, 0 for the rows left
        out).  One copy to the host (the score rides along as an int32 bit pattern)."""
        import t2v_hip
        live = [b for b, a in enumerate(als) if t2v_hip.mas_feasible(a.size(0), a.size(1), max_step)]
        found = [None] * len(als)
        dev = als[0].device
        width = max(a.size(1) for a in als)
        durations = torch.zeros(len(als), width, device=dev, dtype=torch.int32)
        starts = torch.zeros(len(als), width, device=dev, dtype=torch.int32)
        if not live:
            return found, durations, starts
        n, L = [als[b].size(0) for b in live], [als[b].size(1) for b in live]
        A = torch.zeros(len(live), max(n), max(L), device=dev)
        for k, b in enumerate(live):
            A[k, :n[k], :L[k]] = als[b]
        r = t2v_hip.mas(A, n, L, max_step)
        at = torch.tensor(live, device=dev)
        durations[at, :max(L)] = r.durations
        starts[at, :max(L)] = r.starts
        host = torch.cat([r.durations, r.starts, r.score.view(torch.int32)[:, None]], 1).cpu()
        logp = host[:, 2 * max(L)].contiguous().view(torch.float32).tolist()
        for k, b in enumerate(live):
            found[b] = (host[k, :L[k]].tolist(), host[k, max(L):max(L) + L[k]].tolist(), logp[k])
        return found, durations, starts

    def durations(self, rows, batch_size=8, max_step=1):
        """How long does each symbol of a recording last?  rows: filelist rows (audio_path, text, speaker, emotion).  The model
        runs teacher-forced on each recording (`_forced_alignments`: one utterance per forward call, eval mode, no gradients)
        and the best monotonic path through its alignments (`t2v_hip.mas`, steps of at most max_step symbols per frame) segments
        the recording into the text's own symbols; only the search is batched, over the alignments of batch_size rows.
        Returns one dict per row, in input order: `durations` and `starts` (host lists of n_symbols frame counts and first
        frames; the durations sum to n_frames), `n_frames`, `n_symbols` and `align_logp`, the mean log attention weight along
        the path (low for a transcript that does not match its audio).  A row whose text has more symbols than its frames can
        reach has None for durations, starts and align_logp.  A row's result does not depend on its group."""
        import t2v_hip
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1, got %r" % (batch_size,))
        if isinstance(max_step, bool) or int(max_step) != max_step or not 1 <= max_step <= t2v_hip.MAS_MAX_STEP:
            raise ValueError("max_step %r must be an integer in 1..%d" % (max_step, t2v_hip.MAS_MAX_STEP))
        if self.model is None:
            raise RuntimeError("durations: no model (load_checkpoint() or load() first)")
        rows = list(rows)
        out = []
        for i0 in range(0, len(rows), batch_size):
            group = rows[i0:i0 + batch_size]
            uniq = list(dict.fromkeys(r[0] for r in group))
            mels, n_uniq = self.load_mels(uniq)
            als = self._forced_alignments([r[1] for r in group], mels, n_uniq, [uniq.index(r[0]) for r in group])
            for al, found in zip(als, self._search_rows(als, int(max_step))[0]):
                d, s, logp = found or (None, None, None)
                out.append({'durations': d, 'starts': s, 'n_frames': al.size(0), 'n_symbols': al.size(1), 'align_logp': logp})
        return out

    @torch.no_grad()
    def alignment(self, texts, condition_on_ref=False, ref_audios=None, ratios=(1.0, 0.0, 0.0, 0.0), batch_size=8, mas=False,
                  max_step=1):
        """Did the decoder read these sentences?  The texts are synthesised as `synthesize_batch` does (same conditioning
        arguments, batch_size texts at a time, in input order, the decoder's seeds as len(texts) synthesize() calls) and
        their alignments scored by `t2v_hip.alignment_stats`.  Returns one dict per text: evaluation.ALIGNMENT_KEYS,
        `n_frames`, and `durations`, a host list of n_symbols frame counts: how many frames attended each text symbol most
        (the histogram of the argmax path; it sums to n_frames).  mas=True adds `mas_durations`, the frames per symbol along
        the best monotonic path through the same alignments (`t2v_hip.mas` with steps of at most max_step: a segmentation,
        which the histogram is not), and `align_logp`, the mean log weight along it; both None for a text with more symbols
        than its frames can reach."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1, got %r" % (batch_size,))
        if self.model is None:
            raise RuntimeError("alignment: no model (load_checkpoint() or load() first)")
        texts = list(texts)
        if condition_on_ref and (ref_audios is None or len(ref_audios) != len(texts)):
            raise ValueError("condition_on_ref needs one reference audio per text")
        per_text = len(ratios) and not np.isscalar(ratios[0])
        if per_text and len(ratios) != len(texts):
            raise ValueError("ratios: %d tuples for %d texts" % (len(ratios), len(texts)))
        out = []
        for i0 in range(0, len(texts), batch_size):
            chunk = texts[i0:i0 + batch_size]
            _, _, _, al, n_frames, lens = self._synthesize_ragged(
                chunk, condition_on_ref, ref_audios[i0:i0 + batch_size] if condition_on_ref else None,
                list(ratios[i0:i0 + batch_size]) if per_text else ratios)
            n = n_frames.tolist()
            fields, paths = self._alignment_rows(al, n, lens, with_path=True)
            if mas:
                forced = self._search_rows([al[b, :n[b], :lens[b]] for b in range(len(chunk))], max_step)[0]
            for b, f in enumerate(fields):
                f['n_frames'] = n[b]
                f['durations'] = torch.bincount(paths[b, :n[b]].long(), minlength=lens[b]).tolist()
                if mas:
                    f['mas_durations'], _, f['align_logp'] = forced[b] or (None, None, None)
                out.append(f)
        return out

    @torch.no_grad()
    def evaluate(self, rows, batch_size=8, condition='ref', prosody=False, alignment=False, style=False, style_k=5, aligned=False,
                 energy=False, voice=False, durations=False, max_step=1, rhythm=None, rhythm_window=None):
        """Score filelist rows (audio_path, text, speaker, emotion) by free-running synthesis: each text is synthesised
        (`synthesize_batch`, batch_size rows at a time, in input order) and compared with its own recording.  condition='ref':
        the style comes from that recording (copy synthesis; its mel is computed once, for the style and for the comparison);
        'emotion': from the centroid of the row's emotion label, which needs `load()`.  The decoder consumes its seeds as
        len(rows) consecutive synthesize() calls.  Returns one record per row, in input order: the fields of `scoring.plain`
        and those of every score that is on, each a function of scoring.py whose docstring says what it computes; the scores
        combine freely, and a score that is off leaves every record and summary with exactly the keys it held.
        alignment: `scoring.alignment`, evaluation.ALIGNMENT_KEYS.
        prosody, energy, voice: `scoring.prosody`, evaluation.PROSODY_KEYS, `scoring.energy`, evaluation.ENERGY_KEYS, and
        `scoring.voice`, evaluation.VOICE_KEYS.  They need the Griffin-Lim vocoder, which runs once per group for the three
        (`scoring.Group`) with the np.random draws of `synthesize_batch(paths=...)`; any of them alone draws what the others
        would.  A row decoded to fewer than the vocoder's 4 frames has no waveform, and None on its synthesised side.
        aligned: `scoring.aligned`, evaluation.ALIGNED_KEYS; mcd_db and warp_dev need no vocoder, the six F0 values are None
        without prosody, and with energy evaluation.ENERGY_ALIGNED_KEYS, with voice evaluation.VOICE_ALIGNED_KEYS come with
        it.  With speed or pitch on the vocoder the waveform's tracks lie on another time axis than the mels' warping path:
        aligned together with prosody, energy or voice is then a ValueError.
        durations: `scoring.durations`, evaluation.DURATION_KEYS: the free-running alignments of the synthesis and the
        teacher-forced alignments of the recording, each forced onto the row's text by `t2v_hip.mas` with steps of at most
        max_step; with prosody evaluation.DURATION_F0_KEYS come with it, and with speed or pitch on the vocoder the two together
        are the ValueError of aligned, for its reason.  The teacher-forced passes take no decoder seed.
        style: `scoring.style_mu` per group and `scoring.style_records` after the last, evaluation.STYLE_KEYS; None for a row
        decoded to fewer than the encoder's 2 frames.  style_k is lowered to (distinct recordings - 1) when there are too few;
        fewer than 2 distinct recordings, or one path under two labels, is a ValueError.  The result is then an
        evaluation.StyleRecords: the same list, with `style_info` for `evaluation.summarize`.
        rhythm: None, or 'ref': every synthesis is decoded along the symbol durations of its own recording (`rhythm_plan` with
        rhythm_from = the row's wav, rhythm_window around each planned symbol), which takes rhythm out of the comparison: the
        synthesis has the recording's frame count, and what is left in the scores is not timing.  Every record then holds
        'rhythm': 'ref'; without it the records hold the keys they held.  A recording whose text has more symbols than its
        frames can reach is a ValueError naming the row."""
        import scoring
        import t2v_hip
        if condition not in ('ref', 'emotion'):
            raise ValueError("condition must be 'ref' or 'emotion', got %r" % (condition,))
        if rhythm not in (None, 'ref'):
            raise ValueError("rhythm must be None or 'ref', got %r" % (rhythm,))
        if rhythm is None and rhythm_window is not None:
            raise ValueError("rhythm_window acts on a plan: give rhythm='ref'")
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1, got %r" % (batch_size,))
        if self.model is None:
            raise RuntimeError("evaluate: no model (load_checkpoint() or load() first)")
        if condition == 'emotion' and self.neu is None:
            raise RuntimeError("evaluate(condition='emotion') needs the emotion centroids: use load(), not load_checkpoint()")
        if prosody:
            self._need_griffin_lim('evaluate(prosody=True)')
        if energy:
            self._need_griffin_lim('evaluate(energy=True)')
        if voice:
            self._need_griffin_lim('evaluate(voice=True)')
        if aligned and (prosody or energy or voice) and (self.vocoder.stretch[0] != self.vocoder.stretch[1]
                                                         or self.vocoder.shift[0] != self.vocoder.shift[1]):
            raise ValueError("evaluate(aligned=True) with prosody, energy or voice compares tracks frame by frame along the mels' "
                             "path, and the vocoder's speed %g / pitch %g put its waveform on another time axis: use one or the other"
                             % (self.vocoder.speed, self.vocoder.pitch))
        if durations:
            if isinstance(max_step, bool) or int(max_step) != max_step or not 1 <= max_step <= t2v_hip.MAS_MAX_STEP:
                raise ValueError("max_step %r must be an integer in 1..%d" % (max_step, t2v_hip.MAS_MAX_STEP))
            if prosody and (self.vocoder.stretch[0] != self.vocoder.stretch[1] or self.vocoder.shift[0] != self.vocoder.shift[1]):
                raise ValueError("evaluate(durations=True) with prosody reads the pitch track over the frames of the alignments' "
                                 "path, and the vocoder's speed %g / pitch %g put its waveform on another time axis: use one or "
                                 "the other" % (self.vocoder.speed, self.vocoder.pitch))
        if energy:
            t2v_hip.kweight_coefficients(self.hparams.sampling_rate)        # an unsupported rate is refused before any work
            self._need_frame_grid('evaluate(energy=True)')
        if prosody:
            self._need_tracker_grid('evaluate(prosody=True)')
        if voice:
            self._need_voice_grid('evaluate(voice=True)')
        rows = [(r[0], r[1], r[2], int(r[3])) for r in rows]
        one_hot = {0: (1.0, 0.0, 0.0, 0.0), 1: (0.0, 1.0, 0.0, 0.0), 2: (0.0, 0.0, 0.0, 1.0), 3: (0.0, 0.0, 1.0, 0.0)}
        for row in rows:                    # ratio order (neu, sad, hap, ang), label order EMOTIONS
            if row[3] not in one_hot:
                raise ValueError("emotion label %r outside 0..3" % (row[3],))
        if style:       # the recordings' labels, and the mu of the recordings (by path) and of the synthesised rows as they come
            rec_label, rec_mu, syn_mu = scoring.style_recordings(rows, style_k), {}, []
        records = []
        for i0 in range(0, len(rows), batch_size):
            group = rows[i0:i0 + batch_size]
            paths, texts = [row[0] for row in group], [row[1] for row in group]
            uniq = list(dict.fromkeys(paths))
            wavs = self.load_wavs(uniq)
            mels = self._mels_of(*wavs)
            timing = dict(rhythm=dict(rhythm_from=paths, rhythm_window=rhythm_window)) if rhythm else {}
            if condition == 'ref':
                synthesis = self._synthesize_ragged(texts, True, paths, (1.0, 0.0, 0.0, 0.0), mels, **timing)
            else:
                synthesis = self._synthesize_ragged(texts, False, None, [one_hot[row[3]] for row in group], **timing)
            g = scoring.Group(self, group, synthesis, uniq, wavs, mels, waveforms=prosody or energy or voice)
            parts = [scoring.plain(g)]
            if alignment:
                parts.append(scoring.alignment(g))
            if prosody:
                parts.append(scoring.prosody(g))
            if energy:
                parts.append(scoring.energy(g))
            if voice:
                parts.append(scoring.voice(g))
            if aligned:
                parts.append(scoring.aligned(g, f0=prosody, energy=energy, voice=voice))
            if durations:
                parts.append(scoring.durations(g, int(max_step), f0=prosody))
            if rhythm:
                parts.append([{'rhythm': rhythm}] * len(group))
            if style:
                syn_mu += scoring.style_mu(g, rec_mu)
            records += [{k: v for fields in parts for k, v in fields[b].items()} for b in range(len(group))]
        return scoring.style_records(rows, records, rec_label, rec_mu, syn_mu, style_k) if style else records


# ---------------------------------------------------------------------- command line
DEFAULT_BATCH_SIZE = 8


def add_weights_argument(p):
    """--weights of the three command lines that load a checkpoint (synthesizer.py, evaluate.py, extract_latents.py)"""
    p.add_argument('--weights', choices=sorted(WEIGHTS), default=None,
                   help="which weights of the checkpoint: raw (default) = the last iteration's, ema = the moving average a "
                        "run with hparams.ema_decay > 0 keeps beside them")


def weights_option(args):
    """the load / load_checkpoint keyword of --weights: nothing without the flag, so the call is the one it always was"""
    return {} if args.weights is None else {'weights': args.weights}


def build_arg_parser():
    """The reference's flags where they exist (synthesizer.py:171-179: --load_path, --sample_path, --text) and the batched
    front end's own."""
    import argparse
    p = argparse.ArgumentParser(description="text -> <sample_path>/<i>.wav (or <i>.npy mels without a vocoder)")
    p.add_argument('--load_path', required=True, help="checkpoint written by train.py")
    p.add_argument('--sample_path', default="samples")
    p.add_argument('--text', action='append', default=[], help="a sentence (repeatable)")
    p.add_argument('--text_file', default=None, help="one sentence per line (after the --text sentences)")
    p.add_argument('--batch_size', type=int, default=DEFAULT_BATCH_SIZE, help="texts per synthesize_batch call")
    p.add_argument('--vocoder', choices=list(VOCODERS), default=None,
                   help="without it the post-net mels are written; griffin_lim_fast: momentum 0.99 and NNLS mel inversion; "
                        "spsi: NNLS and the phase from the magnitudes' peaks, no iterations (low voices stay voiced)")
    p.add_argument('--ratios', default='1,0,0,0', help="emotion mix neu,sad,hap,ang")
    p.add_argument('--ref_audio', default=None, help="condition every text on this reference wav instead of --ratios")
    p.add_argument('--filelist_path', default='./web/static/uploads/koemo_spk_emo_all_test.txt',
                   help="reference utterances of the emotion centroids (or their cache next to the checkpoint)")
    from evaluation import parse_attention_window
    p.add_argument('--attention_window', type=parse_attention_window, default=None, metavar='BACK,AHEAD',
                   help="attention constraint: every frame attends within BACK positions behind and AHEAD in front of the "
                        "position the previous frame attended most (default: none)")
    p.add_argument('--hparams', default='', help="comma separated name=value overrides")
    add_weights_argument(p)
    from wavio import add_wav_arguments
    add_wav_arguments(p)
    add_tempo_arguments(p)
    add_rhythm_arguments(p)
    return p


def add_rhythm_arguments(p):
    """--rhythm_from, --durations, --rhythm_scale and --rhythm_window: decode along a duration plan (Synthesizer.rhythm_plan)"""
    from evaluation import parse_attention_window
    p.add_argument('--rhythm_from', default=None, metavar='WAV',
                   help="say every text with the timing of this recording of the same text: its symbol durations, measured by "
                        "forced alignment, become the decoder's plan")
    p.add_argument('--durations', default=None, metavar='FILE.npz',
                   help="frames per symbol as extract_durations.py writes them, row i for text i")
    p.add_argument('--rhythm_scale', type=float, default=1.0, metavar='R',
                   help="factor on every planned duration (2 is twice as slow); needs --rhythm_from or --durations")
    p.add_argument('--rhythm_window', type=parse_attention_window, default=None, metavar='BACK,AHEAD',
                   help="positions the decoder may look behind and in front of the planned symbol (default 1,1, an "
                        "uncalibrated choice; 0,0 reads exactly the planned symbol)")


def read_durations(path, n_texts):
    """the rows of an extract_durations.py file as a list of n_texts float32 arrays; SystemExit when the file has another
    number of rows or a row without a path (durations -1)"""
    with np.load(path) as z:
        offsets, durations = z['offsets'], z['durations']
    if len(offsets) - 1 != n_texts:
        raise SystemExit("--durations: %s holds %d rows for %d texts" % (path, len(offsets) - 1, n_texts))
    rows = [durations[offsets[i]:offsets[i + 1]].astype(np.float32) for i in range(n_texts)]
    for i, r in enumerate(rows):
        if r.size and r.min() < 0:
            raise SystemExit("--durations: row %d of %s has no path (its durations are -1)" % (i, path))
    return rows


def add_tempo_arguments(p):
    """--speed and --pitch of the synthesis command lines: what the built-in vocoder writes (GriffinLimVocoder(speed=, pitch=))"""
    p.add_argument('--speed', type=float, default=1.0, metavar='R',
                   help="speaking rate of the built-in vocoder's output, 0.25..4 (default 1: unchanged)")
    p.add_argument('--pitch', type=float, default=0.0, metavar='ST',
                   help="pitch shift of the built-in vocoder's output in semitones, -12..12 (default 0: unchanged)")
    p.add_argument('--formant', type=float, default=0.0, metavar='ST',
                   help="shift of the spectral envelope (the formants) of the built-in vocoder's output in semitones, -12..12; the "
                        "harmonics stay (default 0: unchanged)")
    p.add_argument('--preserve_formants', action='store_true',
                   help="--pitch moves F0 alone and leaves the formants where they were (default: they move with the pitch)")


def tempo_options(args):
    """the Synthesizer keywords of add_tempo_arguments' flags (formant and preserve_formants only when their flags are used);
    SystemExit on a value out of range"""
    import t2v_hip
    try:
        t2v_hip.vocoder_rates(args.speed, args.pitch)
    except ValueError as e:
        raise SystemExit("--speed / --pitch: %s" % e)
    out = {'speed': args.speed, 'pitch': args.pitch}
    try:
        t2v_hip.vocoder_warp(args.pitch, args.formant, args.preserve_formants)
    except ValueError as e:
        raise SystemExit("--formant / --preserve_formants: %s" % e)
    if args.formant != 0.0:
        out['formant'] = args.formant
    if args.preserve_formants:
        out['preserve_formants'] = True
    return out


def parse_args(argv=None):
    args = build_arg_parser().parse_args(argv)
    ratios = tuple(float(x) for x in args.ratios.split(','))
    if len(ratios) != 4:
        raise SystemExit("--ratios takes four comma separated numbers, got %r" % args.ratios)
    args.ratios = ratios
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    texts = list(args.text)
    if args.text_file:
        with open(args.text_file, encoding='utf-8') as f:
            texts += [line.strip() for line in f if line.strip()]
    if not texts:
        raise SystemExit("no text: give --text and/or --text_file")
    args.texts = texts
    if (args.speed != 1.0 or args.pitch != 0.0) and args.vocoder is None:
        raise SystemExit("--speed / --pitch act in the built-in vocoder: give --vocoder")
    if (args.formant != 0.0 or args.preserve_formants) and args.vocoder is None:
        raise SystemExit("--formant / --preserve_formants act in the built-in vocoder: give --vocoder")
    tempo_options(args)
    if args.rhythm_from is not None and args.durations is not None:
        raise SystemExit("--rhythm_from and --durations both set the plan: give one")
    if args.rhythm_from is None and args.durations is None and (args.rhythm_scale != 1.0 or args.rhythm_window is not None):
        raise SystemExit("--rhythm_scale / --rhythm_window act on a plan: give --rhythm_from or --durations")
    if not args.rhythm_scale > 0.0:
        raise SystemExit("--rhythm_scale must be > 0")
    return args


def main(argv=None):
    from wavio import wav_options
    args = parse_args(argv)
    hp = create_hparams()
    hp.sampling_rate = 16000                 # the reference's Synthesizer() overrides (synthesizer.py:47-51)
    hp.max_decoder_steps = 600
    if args.hparams:
        hp.parse(args.hparams)
    syn = Synthesizer(hp, attention_window=args.attention_window, **tempo_options(args), **wav_options(args)).load(args.load_path, vocoder=args.vocoder, filelist_path=args.filelist_path, **weights_option(args))
    os.makedirs(args.sample_path, exist_ok=True)
    texts = args.texts
    planned = read_durations(args.durations, len(texts)) if args.durations is not None else None
    for i0 in range(0, len(texts), args.batch_size):
        chunk = texts[i0:i0 + args.batch_size]
        paths = [os.path.join(args.sample_path, str(i0 + j) + ('.wav' if syn.vocoder is not None else '')) for j in range(len(chunk))]
        rhythm = {}                                 # without the rhythm flags the call is the one it always was
        if planned is not None:
            rhythm = dict(durations=planned[i0:i0 + len(chunk)])
        elif args.rhythm_from is not None:
            rhythm = dict(rhythm_from=[args.rhythm_from] * len(chunk))
        if rhythm:
            rhythm.update(rhythm_scale=args.rhythm_scale, rhythm_window=args.rhythm_window)
        syn.synthesize_batch(chunk, paths, args.ref_audio is not None,
                             [args.ref_audio] * len(chunk) if args.ref_audio else None, args.ratios, **rhythm)
        for p in paths:
            print(p if syn.vocoder is not None else p + '.npy')


if __name__ == "__main__":
    main()
