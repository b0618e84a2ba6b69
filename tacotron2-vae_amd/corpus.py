"""The training set resident on the GPU (train.py --resident_corpus, off by default).

ResidentCorpus turns every utterance of its filelists into a log-mel once, with the front-end kernel DeviceFrontendCollate
runs per batch, and keeps mels, symbol ids and labels in device memory; ResidentCollate then assembles a batch from a list of
utterance indices with ONE launch (csrc/collate.hip, t2v_collate_batch).  Per batch the host sorts B integers and uploads
them: no wav is opened, no text is tokenised, nothing is padded on the host.  The batches are those of DeviceFrontendCollate
on TextMelLoader(return_audio=True) items, bit for bit.
"""
import random
import time
import wave

import numpy as np
import torch
import torch.utils.data

from utils import load_filepaths_and_text


class CorpusView(torch.utils.data.Dataset):
    """Filelist k of a ResidentCorpus as a Dataset: an item is the utterance's GLOBAL index (a Python int), so DataLoader,
    DistributedSampler, BucketBatchSampler and validate() work unchanged and the collate gets a list of indices."""

    def __init__(self, corpus, k):
        self.corpus, self.k = corpus, int(k)
        self.start, self.stop = corpus.bounds[self.k], corpus.bounds[self.k + 1]

    def __len__(self):
        return self.stop - self.start

    def __getitem__(self, index):
        index = int(index)
        if index < 0:
            index += len(self)
        if not 0 <= index < len(self):
            raise IndexError("utterance %d of a filelist of %d" % (index, len(self)))
        return self.start + index

    def lengths(self):
        """TextMelLoader.lengths() from the tables: mel frames of every entry"""
        return [int(n) for n in self.corpus.n_frames[self.start:self.stop]]

    def text_lengths(self):
        """TextMelLoader.text_lengths() from the tables: symbols of every entry"""
        return [int(n) for n in self.corpus.n_ids[self.start:self.stop]]


class ResidentCorpus(object):
    """Several filelists (training, validation) in one store: validate() builds its own DataLoader from `valset` and the SAME
    collate_fn, so one collate object serves every list and an item is a global index.

    Host tables (built without a GPU), one entry per filelist row `path|text|speaker|emotion` in the order TextMelLoader gives it
    (each list shuffled once with random.seed(1234), reference data_utils.py:29-30): ids (list of int32 arrays), n_ids, n_samples,
    n_frames = n_samples // hop + 1, speaker, emotion (int64 arrays), paths, rows (the line of the filelist, from 1) and
    bounds (list k holds the global indices bounds[k] .. bounds[k + 1]).  Everything that comes from outside is checked while the
    tables are built; each error names the file and the row.

    build=True also builds the device store (t2v_hip.CorpusStore), once: the audio goes through
    TacotronSTFT.mel_spectrogram(int16 batch, lengths=, scale=1/max_wav_value) in groups, the call DeviceFrontendCollate makes,
    and every utterance's (80, T_i) is written at its offset of one flat fp32 buffer.  The audio is not kept.  The store must
    take no more than MAX_FREE_FRACTION of the free device memory: otherwise building is a ValueError that names
    device_frontend=True, the loader that holds one batch at a time."""

    MAX_FREE_FRACTION = 0.5     # of torch.cuda.mem_get_info()'s free bytes; a condition, not a tuning knob
    GROUP_SAMPLES = 1 << 23     # int16 samples of one front-end launch while building, padding included (16 MB of audio)
    N_MEL = 80

    def __init__(self, filelists, hparams, stft=None, build=True):
        from text import text_to_sequence
        t0 = time.perf_counter()
        if isinstance(filelists, str):
            filelists = [filelists]
        self.filelists = list(filelists)
        self.hop = int(hparams.hop_length)
        self.scale = 1.0 / hparams.max_wav_value
        self.sampling_rate = int(hparams.sampling_rate)
        self.n_symbols = int(hparams.n_symbols)
        self.n_speakers, self.n_emotions = int(hparams.n_speakers), int(hparams.n_emotions)
        self.hparams = hparams
        self.paths, self.rows, self.ids, self.bounds = [], [], [], [0]
        n_ids, n_samples, speaker, emotion = [], [], [], []
        for filelist in self.filelists:
            entries = list(enumerate(load_filepaths_and_text(filelist), 1))
            random.seed(1234)
            random.shuffle(entries)     # the permutation TextMelLoader draws: it depends on the length of the list alone
            for row, fields in entries:
                where = "%s row %d" % (filelist, row)
                if len(fields) < 4:
                    raise ValueError("%s: `path|text|speaker|emotion` expected, got %d field(s)" % (where, len(fields)))
                path, text = fields[0], fields[1]
                where = "%s (%s)" % (where, path)
                ids = np.asarray(text_to_sequence(text, hparams.text_cleaners), dtype=np.int64)
                if ids.size == 0:
                    raise ValueError("%s: the text has no symbols" % where)
                speaker.append(self._label(fields[2], self.n_speakers, 'speaker', where))
                emotion.append(self._label(fields[3], self.n_emotions, 'emotion', where))
                n_samples.append(self._sample_count(path, where))
                self.paths.append(path)
                self.rows.append(row)
                self.ids.append(ids.astype(np.int32))
                n_ids.append(ids.size)
            self.bounds.append(len(self.paths))
        if not self.paths:
            raise ValueError("ResidentCorpus: no utterances in %s" % ', '.join(self.filelists))
        self._check_ids()
        self.n_ids = np.asarray(n_ids, dtype=np.int64)
        self.n_samples = np.asarray(n_samples, dtype=np.int64)
        self.n_frames = self.n_samples // self.hop + 1
        self.speaker = np.asarray(speaker, dtype=np.int64)
        self.emotion = np.asarray(emotion, dtype=np.int64)
        self.store = None
        self.build_seconds = time.perf_counter() - t0       # the tables; build_store() adds the device store's share
        if build:
            self.build_store(stft)

    def __len__(self):
        return len(self.paths)

    def view(self, k):
        return CorpusView(self, k)

    # -- checks of outside input
    def _check_ids(self):
        """the IndexError of BatchLayout.check_ids, raised here because the collate hands parse_batch DEVICE ids, which that
        check does not look at.  One comparison over all ids; the offending row is looked for only when it fails."""
        ids = np.concatenate(self.ids)
        if ids.min() >= 0 and ids.max() < self.n_symbols:
            return
        from model import BatchLayout
        layout = type('_CorpusLayout', (BatchLayout,), {'n_symbols': self.n_symbols})
        for i, row_ids in enumerate(self.ids):
            try:
                layout.check_ids(torch.from_numpy(row_ids))
            except IndexError as e:
                raise IndexError("%s row %d (%s): %s" % (self._filelist_of(i), self.rows[i], self.paths[i], e))

    @staticmethod
    def _label(field, width, what, where):
        try:
            index = int(field)
        except ValueError:
            raise ValueError("%s: the %s index %r is not an integer" % (where, what, field))
        if not 0 <= index < width:
            raise ValueError("%s: %s index %d outside the one-hot width %d" % (where, what, index, width))
        return index

    def _sample_count(self, path, where):
        """from the wav header alone (what TextMelLoader.lengths() reads)"""
        try:
            with wave.open(path, 'rb') as w:
                sr, width, channels, n = w.getframerate(), w.getsampwidth(), w.getnchannels(), w.getnframes()
        except wave.Error as e:
            raise ValueError("%s: not a 16-bit PCM wav (%s)" % (where, e))
        if sr != self.sampling_rate:
            raise ValueError("{} SR doesn't match target {} SR ({})".format(sr, self.sampling_rate, where))
        if width != 2:
            raise ValueError("%s: the device front end takes 16-bit PCM, the file has %d-bit samples" % (where, 8 * width))
        if channels != 1:
            raise ValueError("%s: one channel expected, the file has %d" % (where, channels))
        if n <= 512:
            raise ValueError("%s: %d samples; the front end's reflect padding needs more than 512" % (where, n))
        return n

    # -- the device store
    def store_bytes(self):
        """bytes of device memory the store takes (the transient audio of one group while building is not counted)"""
        n = len(self)
        return 4 * self.N_MEL * int(self.n_frames.sum()) + 4 * int(self.n_ids.sum()) + n * (2 * 8 + 4 * 4)

    def _read_pcm(self, i):
        from scipy.io.wavfile import read
        where = "%s row %d (%s)" % (self._filelist_of(i), self.rows[i], self.paths[i])
        sr, data = read(self.paths[i])
        if data.dtype != np.int16 or data.ndim != 1 or data.shape[0] != self.n_samples[i] or sr != self.sampling_rate:
            raise ValueError("%s: the samples do not match the wav header (16-bit mono PCM of %d samples at %d Hz expected)"
                             % (where, self.n_samples[i], self.sampling_rate))
        return data

    def _filelist_of(self, i):
        for k in range(len(self.filelists)):
            if i < self.bounds[k + 1]:
                return self.filelists[k]
        raise IndexError(i)

    def build_store(self, stft=None):
        import t2v_hip
        if int(self.hparams.n_mel_channels) != self.N_MEL:
            raise ValueError("resident_corpus: the store and t2v_collate_batch hold %d mel channels, hparams.n_mel_channels is %d"
                             % (self.N_MEL, self.hparams.n_mel_channels))
        if not torch.cuda.is_available():
            raise t2v_hip.T2VHipError("ResidentCorpus needs a GPU: the store lives in device memory")
        t0 = time.perf_counter()
        need = self.store_bytes()
        free = torch.cuda.mem_get_info()[0]
        if need > self.MAX_FREE_FRACTION * free:
            raise ValueError("resident_corpus: the store needs %.1f MB, more than %g of the %.1f MB of free device memory; "
                             "use device_frontend=True instead, which keeps one batch at a time on the device"
                             % (need / 1e6, self.MAX_FREE_FRACTION, free / 1e6))
        if stft is None:
            import layers
            hp = self.hparams
            stft = layers.TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_mel_channels, hp.sampling_rate,
                                       hp.mel_fmin, hp.mel_fmax)
        dev = torch.device('cuda')
        n = len(self)
        mel_off = np.zeros(n, dtype=np.int64)
        mel_off[1:] = np.cumsum(self.N_MEL * self.n_frames)[:-1]
        id_off = np.zeros(n, dtype=np.int64)
        id_off[1:] = np.cumsum(self.n_ids)[:-1]
        mel = torch.empty(self.N_MEL * int(self.n_frames.sum()), dtype=torch.float32, device=dev)
        lo = 0
        while lo < n:       # groups in table order: at least one utterance, then as many as stay under GROUP_SAMPLES with padding
            hi, longest = lo + 1, int(self.n_samples[lo])
            while hi < n and max(longest, int(self.n_samples[hi])) * (hi + 1 - lo) <= self.GROUP_SAMPLES:
                longest = max(longest, int(self.n_samples[hi]))
                hi += 1
            wav = torch.zeros(hi - lo, longest, dtype=torch.int16)
            for g, i in enumerate(range(lo, hi)):
                wav[g, :self.n_samples[i]] = torch.from_numpy(np.ascontiguousarray(self._read_pcm(i)))
            out = stft.mel_spectrogram(wav.to(dev), lengths=torch.from_numpy(self.n_samples[lo:hi].copy()), scale=self.scale)
            for g, i in enumerate(range(lo, hi)):
                t = int(self.n_frames[i])
                mel[mel_off[i]:mel_off[i] + self.N_MEL * t].view(self.N_MEL, t).copy_(out[g, :, :t])
            lo = hi
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.store = t2v_hip.CorpusStore(
            self.n_speakers, self.n_emotions, torch.from_numpy(self.n_frames), torch.from_numpy(self.n_ids),
            mel=mel, mel_off=torch.from_numpy(mel_off).to(dev), n_frames=i32(self.n_frames),
            ids=i32(np.concatenate(self.ids)), id_off=torch.from_numpy(id_off).to(dev), n_ids=i32(self.n_ids),
            speaker=i32(self.speaker), emotion=i32(self.emotion))
        torch.cuda.synchronize()
        self.build_seconds += time.perf_counter() - t0
        return self.store

    def describe(self):
        """the start-up line of train.py"""
        return ("Resident corpus: {} utterances, {} frames, {:.1f} MB on the device, built in {:.2f} s".format(
            len(self), int(self.n_frames.sum()), self.store_bytes() / 1e6, self.build_seconds))


class ResidentCollate(object):
    """collate_fn over a ResidentCorpus: a list of global utterance indices -> the reference's 7-tuple, ordered and padded like
    TextMelCollate / DeviceFrontendCollate.  input_lengths stays the CPU LongTensor the sort returns (parse_batch reads max_len
    from it without waiting for the device); the other six are device tensors written by one t2v_collate_batch launch on the
    current stream.  Nothing here reads device memory back.

    The ordered indices reach the device through a ring of pinned slots and an asynchronous copy, like t2v_hip.StepParams.  The
    host runs ahead of the GPU, so a slot must not be rewritten before its copy has executed: every slot carries the event
    recorded behind its last copy and is waited for before it is written again.  With RING slots that wait only ever blocks a
    host that is RING batches ahead of the device (the training engine keeps it within two steps)."""

    RING = 8

    def __init__(self, corpus, hparams):
        self.corpus = corpus
        self.n_frames_per_step = int(hparams.n_frames_per_step)
        self._slots = self._events = None
        self._i = 0

    def plan(self, batch):
        """the host side of a batch, from the tables alone: (input_lengths (CPU LongTensor, descending), the global indices in
        row order, T_in, T_out).  torch.sort on the symbol counts in the batch's order is the very call the two other collates
        make on the same values, so ties fall the same way."""
        c = self.corpus
        batch = [int(i) for i in batch]
        if not batch or min(batch) < 0 or max(batch) >= len(c):
            raise ValueError("ResidentCollate: utterance indices must lie in [0, %d), got %s" % (len(c), batch))
        input_lengths, order = torch.sort(torch.LongTensor([int(c.n_ids[i]) for i in batch]), dim=0, descending=True)
        rows = [batch[src] for src in order.tolist()]
        max_t = max(int(c.n_frames[i]) for i in rows)
        r = self.n_frames_per_step
        if max_t % r:
            max_t += r - max_t % r
        return input_lengths, rows, int(input_lengths[0]), max_t

    def _upload(self, rows):
        n = len(rows)
        if self._slots is None or self._slots.size(1) < n:
            if self._events is not None:
                for ev in self._events:
                    if ev is not None:
                        ev.synchronize()
            self._slots = torch.zeros(self.RING, max(n, 16), dtype=torch.int32).pin_memory()
            self._events = [None] * self.RING
        k = self._i % self.RING
        self._i += 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        slot = self._slots[k, :n]
        slot.copy_(torch.tensor(rows, dtype=torch.int32))
        idx = torch.empty(n, dtype=torch.int32, device=self.corpus.store.mel.device)
        idx.copy_(slot, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[k] = ev
        return idx

    def __call__(self, batch):
        import t2v_hip
        store = self.corpus.store
        if store is None:
            raise t2v_hip.T2VHipError("ResidentCollate: the corpus has no device store (ResidentCorpus(build=True))")
        input_lengths, rows, T_in, T_out = self.plan(batch)
        # plan() has checked the indices against the tables and T_in / T_out are the maxima over these very rows, so
        # t2v_hip.collate_check (the check of a caller that brings its own widths) has nothing left to find here
        text, mel, gate, output_lengths, speakers, emotions = t2v_hip.collate_batch(store, self._upload(rows), T_in, T_out)
        return text, input_lengths, mel, gate, output_lengths, speakers, emotions
