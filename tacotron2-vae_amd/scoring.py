"""The scores of `Synthesizer.evaluate`, one function each, over one `Group` per batch of rows.

The Group holds what the scores share, under one name each: the synthesis and the recordings of the group, which recording
each row is compared with, which rows are long enough for the vocoder and for the reference encoder, the synthesised
waveforms, and the pitch, level and voice-quality tracks of both sides.  Every score is a function of the Group that returns
one dict of fields per row; none reads what another left behind except through the Group."""
from functools import cached_property

import numpy as np
import torch

import evaluation as E                   # its *_fields are looked up at each call
import t2v_hip
from latent_scores import knn_predict, silhouette

VOCODER_MIN_FRAMES = 4       # Griffin-Lim's shortest mel
ENCODER_MIN_FRAMES = 2       # the reference encoder's


def _take(t, idx):
    """the rows idx (ascending, distinct) of t; t itself when they are all of its rows"""
    return t if len(idx) == t.size(0) else t[torch.tensor(idx, device=t.device)]


class Group(object):
    """One batch of evaluate()'s rows.  rows: (audio_path, text, speaker, emotion id); synthesis: what `_synthesize_ragged`
    returned for their texts; uniq: their distinct recordings in order of first appearance, wavs = (y, sample counts) and
    mels = (mels, frame counts) of those.  waveforms: run the vocoder (`vocoder.batch`, which draws its initial phases from
    np.random) on the pre-Postnet mels of the rows that are long enough for it, here, before any score.

    n, n_ref: frame counts of the synthesised rows and of each row's recording; which[b]: the recording of row b, an index into
    uniq (`ref` picks the rows' recordings out of any per-recording tensor); encodable: the rows the reference encoder takes;
    with_wav: the rows that have a waveform (empty without `waveforms`), wav_slot their places among the waveforms, wav_index
    with_wav on the device; y_syn, syn_samples, syn_frames: the waveforms zero-padded in one tensor, their sample counts and the
    frames of their own tracks (n[b] without speed or pitch on the vocoder, else what it wrote); those four are None for a
    group without a waveform.  f0_tracks, loudness, levels, voice: both sides' tracks, made by the first score that asks."""

    def __init__(self, syn, rows, synthesis, uniq, wavs, mels, waveforms=False):
        self.syn, self.rows, self.uniq = syn, rows, uniq
        self.mel, self.mel_postnet, self.gate, self.alignments, self.n_frames, self.lens = synthesis
        (self.y_ref, self.samples_ref), (self.ref_mels, self.n_uniq) = wavs, mels
        self.n = self.n_frames.tolist()
        self.which = [uniq.index(r[0]) for r in rows]
        self._pick = None if self.which == list(range(len(rows))) else torch.tensor(self.which, device=self.ref_mels.device)
        self.n_ref = [self.n_uniq[k] for k in self.which]
        self.encodable = [b for b in range(len(rows)) if self.n[b] >= ENCODER_MIN_FRAMES]
        self.with_wav = [b for b in range(len(rows)) if waveforms and self.n[b] >= VOCODER_MIN_FRAMES]
        self.wav_slot = {b: k for k, b in enumerate(self.with_wav)}
        self.y_syn = self.syn_samples = self.syn_frames = self.wav_index = None
        if self.with_wav:
            found = syn.vocoder.batch(_take(self.mel, self.with_wav), [self.n[b] for b in self.with_wav])
            self.syn_samples = [w.numel() for w in found]
            self.syn_frames = [s // syn.hparams.hop_length + 1 for s in self.syn_samples]
            self.y_syn = torch.zeros(len(found), max(self.syn_samples), device=self.mel.device)
            for k, w in enumerate(found):
                self.y_syn[k, :w.numel()] = w
            self.wav_index = torch.tensor(self.with_wav, device=self.mel.device)

    def ref(self, per_recording):
        """row b of the result is row which[b] of a (len(uniq), ...) tensor"""
        return per_recording if self._pick is None else per_recording[self._pick]

    def _both_sides(self, measure):
        """(measure(y, sample counts) of the recordings, of the waveforms or None when there is none)"""
        return measure(self.y_ref, self.samples_ref), (measure(self.y_syn, self.syn_samples) if self.with_wav else None)

    @cached_property
    def f0_tracks(self):
        """both sides' `t2v_hip.f0`: Hz per frame, on the device"""
        return self._both_sides(t2v_hip.f0)

    @cached_property
    def loudness(self):
        """both sides' `t2v_hip.loudness`"""
        return self._both_sides(lambda y, n: t2v_hip.loudness(y, n, self.syn.hparams.sampling_rate))

    @cached_property
    def levels(self):
        """both sides' K-weighted level in dB per frame, on the device"""
        return tuple(None if r is None else t2v_hip.energy_db(r.frame_ms) for r in self.loudness)

    @cached_property
    def voice(self):
        """both sides' `t2v_hip.voice_quality`"""
        return self._both_sides(t2v_hip.voice_quality)

    def tracks_on_host(self, tracks):
        """per row (its waveform's track or None, its recording's track) as host lists cut to their frames, from both sides'
        per-frame tensors, (rows, frames) or with planes, (rows, planes, frames), which give a list per plane: side by side in
        one tensor, one copy to the host"""
        both = [t for t in tracks if t is not None]
        width = max(t.size(-1) for t in both)
        host = torch.cat([torch.nn.functional.pad(t, (0, width - t.size(-1))) for t in both], 0).cpu().tolist()
        if both[0].dim() == 2:
            def cut(row, frames):
                return row[:frames]
        else:
            def cut(row, frames):
                return [plane[:frames] for plane in row]
        out = []
        for b in range(len(self.rows)):
            k = self.wav_slot.get(b)
            out.append((None if k is None else cut(host[len(self.uniq) + k], self.syn_frames[k]),
                        cut(host[self.which[b]], self.n_ref[b])))
        return out


def plain(g):
    """The fields every record has: dtw, `t2v_hip.mel_dtw` of the post-net mel against the mel of the row's own recording;
    n_frames, n_ref_frames; hit_max (decoding ended at max_decoder_steps, not at the gate; such a row is still scored) and
    emotion (the label id)."""
    dec = g.syn.model.decoder
    dtw = t2v_hip.mel_dtw(g.mel_postnet, g.n, g.ref(g.ref_mels), g.n_ref).cpu().tolist()
    last = g.gate[torch.arange(len(g.rows), device=g.gate.device), (g.n_frames - 1).to(g.gate.device), 0].cpu()
    fired = (torch.sigmoid(last) > dec.gate_threshold).tolist()
    return [{'dtw': dtw[b], 'n_frames': g.n[b], 'n_ref_frames': g.n_ref[b],
             'hit_max': bool(g.n[b] >= dec.max_decoder_steps and not fired[b]), 'emotion': row[3]}
            for b, row in enumerate(g.rows)]


def alignment(g):
    """What the decoder's alignments say about reading the text (evaluation.ALIGNMENT_KEYS): `t2v_hip.alignment_stats` on the
    alignments of the group, one call and one copy to the host.  It combines freely with every other score and either
    condition."""
    return g.syn._alignment_rows(g.alignments, g.n, g.lens)[0]


def prosody(g):
    """The pitch of both sides (evaluation.PROSODY_KEYS): `t2v_hip.f0` on the waveform `synthesize_batch(paths=...)` would have
    written (the vocoder on the pre-Postnet mel, with the same np.random draws) and on the recording's samples, which are the
    ones read for its mel.  A row decoded to fewer than the vocoder's 4 frames has no waveform, and None on its synthesised
    side.  One copy of the tracks to the host; they stay on the device in g.f0_tracks for `aligned`."""
    return [E.prosody_fields(syn_track, ref_track) for syn_track, ref_track in g.tracks_on_host(g.f0_tracks)]


def energy(g):
    """The level of both sides (evaluation.ENERGY_KEYS): `t2v_hip.loudness` on the same two waveforms as `prosody`, which it
    shares (the vocoder runs once per group).  One copy of the frame tracks to the host; they stay on the device in g.levels
    for `aligned`."""
    ref_loud, syn_loud = g.loudness
    fields = []
    for b, (syn_track, ref_track) in enumerate(g.tracks_on_host(g.levels)):
        fields.append(E.energy_fields(None if syn_track is None else syn_loud.integrated[g.wav_slot[b]], syn_track,
                                    ref_loud.integrated[g.which[b]], ref_track))
    return fields


def aligned(g, f0=False, energy=False, voice=False):
    """The frame-aligned scores (evaluation.ALIGNED_KEYS): the cepstra of the post-net mels and of the recordings' mels
    (`t2v_hip.mel_cepstrum`), one `t2v_hip.aligned_scores` call and one copy to the host.  Without f0 every row gets mcd_db and
    warp_dev, None on the six F0 values, and no vocoder is needed; with f0 (prosody is on) g.f0_tracks, cut to n_frames and
    n_ref_frames, feed the same call: a row without a waveform is unvoiced everywhere, keeps None on its F0 values and still
    gets mcd_db.  energy (energy is on) adds `energy_along_path` on the path of the same call, voice (voice is on)
    `voice_along_path`.  It draws nothing."""
    cep = t2v_hip.mel_cepstrum(g.mel_postnet, g.n)
    cep_ref = g.ref(t2v_hip.mel_cepstrum(g.ref_mels, g.n_uniq))
    f0x = f0y = None
    if f0:
        ref_track, syn_track = g.f0_tracks
        f0y = g.ref(torch.nn.functional.pad(ref_track, (0, max(0, max(g.n_ref) - ref_track.size(1)))))
        f0x = torch.zeros(len(g.rows), max(g.n), device=g.mel.device)
        if syn_track is not None:
            width = min(max(g.n), syn_track.size(1))
            f0x[g.wav_index, :width] = syn_track[:, :width]
    scores = t2v_hip.aligned_scores(cep, g.n, cep_ref, g.n_ref, f0x, f0y, return_path=energy or voice)
    host = torch.cat([scores.counts.double(), scores.sums.double()], 1).cpu().tolist()
    n_counts = len(t2v_hip.ALIGNED_COUNTS)
    fields = [E.aligned_fields(host[b][:n_counts], host[b][n_counts:], f0=f0 and b in g.wav_slot) for b in range(len(g.rows))]
    for on, along_path in ((energy, energy_along_path), (voice, voice_along_path)):
        if on:
            for row, more in zip(fields, along_path(g, scores)):
                row.update(more)
    return fields


def energy_along_path(g, scores):
    """evaluation.ENERGY_ALIGNED_KEYS: the two dB tracks of g.levels at the points of the warping path (scores: an
    AlignedScores with its path), compared where both frames sound.  A few index operations on the device and one copy to the
    host; None for a row without a waveform."""
    fields = [dict.fromkeys(E.ENERGY_ALIGNED_KEYS) for _ in g.rows]
    if not g.with_wav:
        return fields
    ref_db, syn_db = g.levels
    neg = float('-inf')

    def sounding(level, counts):
        counts = torch.tensor(counts, device=level.device)
        level = level.masked_fill(torch.arange(level.size(1), device=level.device)[None, :] >= counts[:, None], neg)
        return level > level.amax(1, keepdim=True) - E.ENERGY_FLOOR_DB
    keep = sounding(syn_db, [g.n[b] for b in g.with_wav]), sounding(ref_db, g.n_uniq)
    for b, pairs in _pairs_along_path(g, scores, (syn_db, ref_db), keep):
        fields[b] = E.energy_path_fields(pairs)
    return fields


def _pairs_along_path(g, scores, tracks, keep):
    """(row, [(synthesis, recording) values]) for every row with a waveform: tracks = two per-frame tensors, of the rows with
    a waveform and of the recordings, read at the points of the warping path (scores: an AlignedScores with its path) where
    keep, two bool tensors of the same shapes, holds on both sides.  A few index operations on the device and one copy to the
    host."""
    dev, sel = tracks[0].device, g.wav_index
    n_x = torch.tensor([g.n[b] for b in g.with_wav], device=dev)
    n_y = torch.tensor([g.n_ref[b] for b in g.with_wav], device=dev)
    path = scores.path[sel].long()
    pi = torch.minimum(path[:, :, 0].clamp(min=0), n_x[:, None] - 1)
    pj = torch.minimum(path[:, :, 1].clamp(min=0), n_y[:, None] - 1)
    a, c = tracks[0].gather(1, pi), g.ref(tracks[1])[sel].gather(1, pj)
    both = (keep[0].gather(1, pi) & g.ref(keep[1])[sel].gather(1, pj)
            & (torch.arange(path.size(1), device=dev)[None, :] < scores.n_points[sel][:, None]))
    host = torch.stack([a.double(), c.double(), both.double()], 1).cpu().tolist()
    for k, b in enumerate(g.with_wav):
        pa, pc, pk = host[k]
        yield b, [(u, v) for u, v, w in zip(pa, pc, pk) if w]


def durations(g, max_step=1, f0=False):
    """The timing per symbol of both sides (evaluation.DURATION_KEYS): `t2v_hip.mas` forces the free-running alignments the
    group already holds onto each row's text, and the teacher-forced alignments of the row's recording against the same text
    (`Synthesizer._forced_alignments`: one forward per row, no decoder seed taken) onto the same symbols; one search call and
    one copy to the host per side.  A side whose text has more symbols than its frames can reach has no path, and None.  f0
    (prosody is on) adds evaluation.DURATION_F0_KEYS: `t2v_hip.segment_means` of g.f0_tracks over the voiced frames of each
    symbol's segment, both sides, one more copy to the host; None for a row without a waveform or without a path.  It draws
    nothing."""
    B = len(g.rows)
    syn_found, syn_dur, syn_start = g.syn._search_rows([g.alignments[b, :g.n[b], :g.lens[b]] for b in range(B)], max_step)
    rec_als = g.syn._forced_alignments([row[1] for row in g.rows], g.ref_mels, g.n_uniq, g.which)
    rec_found, rec_dur, rec_start = g.syn._search_rows(rec_als, max_step)
    none = (None, None, None)
    fields = [E.duration_fields((syn_found[b] or none)[0], (rec_found[b] or none)[0], (syn_found[b] or none)[2],
                                (rec_found[b] or none)[2]) for b in range(B)]
    if not f0:
        return fields
    for row in fields:
        row.update(dict.fromkeys(E.DURATION_F0_KEYS))
    if not g.with_wav:
        return fields
    ref_track, syn_track = g.f0_tracks
    f0y = g.ref(ref_track).contiguous()
    f0x = torch.zeros(B, max(g.n), device=g.mel.device)
    width = min(max(g.n), syn_track.size(1))
    f0x[g.wav_index, :width] = syn_track[:, :width]
    seg_x = t2v_hip.segment_means(f0x, f0x > 0, syn_start, syn_dur)
    seg_y = t2v_hip.segment_means(f0y, f0y > 0, rec_start, rec_dur)
    host = torch.stack([seg_x.sums.double(), seg_x.counts.double(), seg_y.sums.double(), seg_y.counts.double()], 1).cpu().tolist()
    for b in g.with_wav:
        if syn_found[b] is not None and rec_found[b] is not None:
            L = g.lens[b]
            fields[b].update(E.segment_f0_fields(*(plane[:L] for plane in host[b])))
    return fields


def voice(g):
    """The voice quality of both sides (evaluation.VOICE_KEYS): `t2v_hip.voice_quality` on the same two waveforms as `prosody`
    and `energy`, which it shares (the vocoder runs once per group).  One copy of the planes evaluation.VOICE_TRACKS to the
    host; the tracks stay on the device in g.voice for `aligned`.  It draws nothing."""
    stacked = tuple(None if side is None else torch.stack([getattr(side, k) for k in E.VOICE_TRACKS], 1) for side in g.voice)
    named = lambda planes: None if planes is None else dict(zip(E.VOICE_TRACKS, planes))
    return [E.voice_fields(named(syn_planes), named(ref_planes)) for syn_planes, ref_planes in g.tracks_on_host(stacked)]


def voice_along_path(g, scores):
    """evaluation.VOICE_ALIGNED_KEYS: the two alpha_db tracks of g.voice at the points of the warping path, compared where
    both frames are counted (`t2v_hip.voice_counted` of the level_db tracks); None for a row without a waveform."""
    fields = [dict.fromkeys(E.VOICE_ALIGNED_KEYS) for _ in g.rows]
    if not g.with_wav:
        return fields
    ref_vq, syn_vq = g.voice
    keep = (t2v_hip.voice_counted(syn_vq.level_db, [g.n[b] for b in g.with_wav], E.VOICE_FLOOR_DB),
            t2v_hip.voice_counted(ref_vq.level_db, g.n_uniq, E.VOICE_FLOOR_DB))
    for b, pairs in _pairs_along_path(g, scores, (syn_vq.alpha_db, ref_vq.alpha_db), keep):
        fields[b] = E.voice_path_fields(pairs)
    return fields


def style_recordings(rows, style_k):
    """what style=True refuses before any work, and {path: emotion id} of the distinct recordings of rows, in order of first
    appearance"""
    if isinstance(style_k, bool) or int(style_k) != style_k or not 1 <= style_k <= t2v_hip.LATENT_MAX_K:
        raise ValueError("style_k %r must be an integer in 1..%d" % (style_k, t2v_hip.LATENT_MAX_K))
    rec_label = {}
    for row in rows:
        if rec_label.setdefault(row[0], row[3]) != row[3]:
            raise ValueError("evaluate(style=True): %r appears with the emotion labels %d and %d" % (row[0], rec_label[row[0]], row[3]))
    if len(rec_label) < 2:
        raise ValueError("evaluate(style=True) needs at least 2 distinct recordings, got %d" % len(rec_label))
    return rec_label


def style_mu(g, rec_mu):
    """The group's part of the style round trip: the recordings of the group that rec_mu (path -> mu, over the whole call)
    does not hold yet go through the ragged `model.vae_gst` and are added to it; then the post-net mels of the rows the encoder
    takes go through it (eval mode, no random draws).  Returns the rows' mu, None for a row decoded to fewer than the
    encoder's 2 frames.  Nothing is copied to the host here."""
    vae_gst = g.syn.model.vae_gst
    new = [j for j, p in enumerate(g.uniq) if p not in rec_mu]
    if new:
        mu = vae_gst(_take(g.ref_mels, new), [g.n_uniq[j] for j in new])[1]
        rec_mu.update((g.uniq[j], mu[k]) for k, j in enumerate(new))
    out = [None] * len(g.rows)
    if g.encodable:
        mu = vae_gst(_take(g.mel_postnet, g.encodable), [g.n[b] for b in g.encodable])[1]
        for k, b in enumerate(g.encodable):
            out[b] = mu[k]
    return out


def style_records(rows, records, rec_label, rec_mu, syn_mu, style_k):
    """The style round trip (evaluation.STYLE_KEYS) after the last group, from rec_label (`style_recordings`) and the rec_mu and
    syn_mu that `style_mu` collected: one `t2v_hip.latent_neighbours` call places the synthesised rows' mu (None: no style
    fields) among the mu of the distinct recordings, each row's own recording excluded from the vote and taken as the rank's target;
    one more call gives the recordings' own leave-one-out accuracy; host arithmetic in fp64 (latent_scores).  style_k is lowered
    to (distinct recordings - 1) when there are too few.  Returns an evaluation.StyleRecords: the records, with `style_info`
    (k, n_recordings, ref_accuracy) for `evaluation.summarize`."""
    rec_index = {p: j for j, p in enumerate(rec_label)}
    refs = torch.stack([rec_mu[p] for p in rec_label]).float().contiguous()
    labels = np.asarray(list(rec_label.values()), dtype=np.int64)
    k = min(int(style_k), len(rec_label) - 1)
    C = len(E.EMOTIONS)
    loo = t2v_hip.latent_neighbours(refs, labels, k=k, n_classes=C)
    out = E.StyleRecords(records)
    out.style_info = {'k': k, 'n_recordings': len(rec_label),
                      'ref_accuracy': float((knn_predict(loo.idx.cpu().numpy(), labels, C) == labels).mean())}
    have = [i for i, m in enumerate(syn_mu) if m is not None]
    fields = {}
    refs64 = refs.cpu().numpy().astype(np.float64)
    for c0 in range(0, len(have), t2v_hip.LATENT_MAX_POINTS):
        chunk = have[c0:c0 + t2v_hip.LATENT_MAX_POINTS]
        own = [rec_index[rows[i][0]] for i in chunk]
        rows_q = chunk if len(chunk) > 1 else chunk * 2          # the kernel takes 2 queries or more
        own_q = own if len(chunk) > 1 else own * 2
        q = torch.stack([syn_mu[i] for i in rows_q]).float().contiguous()
        near = t2v_hip.latent_neighbours(refs, labels, q, k=k, n_classes=C, exclude=own_q, target=own_q)
        vote = knn_predict(near.idx.cpu().numpy(), labels, C)
        lab = np.asarray([rows[i][3] for i in rows_q], dtype=np.int64)
        sil = silhouette(near.class_sum.cpu().numpy(), near.class_cnt.cpu().numpy(), lab)
        rank = near.rank.cpu().tolist()
        dist = np.sqrt(((q.cpu().numpy().astype(np.float64) - refs64[own_q]) ** 2).sum(axis=1))
        for at, i in enumerate(chunk):
            fields[i] = E.style_fields(rows[i][3], vote[at], rank[at], dist[at], sil[at])
    for i, rec in enumerate(out):
        rec.update(fields.get(i) or E.style_fields(rows[i][3], None, None, None, None))
    return out
