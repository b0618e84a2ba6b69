#!/usr/bin/env python
"""What the data path of `python train.py` costs, on one GPU: the three loaders of train.prepare_dataloaders (host collate,
device_frontend=True, resident_corpus=True) alone and feeding TrainEngine.step, next to the same batches already on the device.

    python tools/bench_data_path.py [--seed 1234] [--utts 600] [--steps 200] [--block 25] [--out FILE]

From the seed it writes `utts` int16 wavs at 16 kHz with koemo's length statistics (symbols per utterance median 71,
mean 84, about 4.6 mel frames per symbol, 389 frames on average) and random Hangul texts into a temporary directory, then, in
ONE process and at the default fp32 batch of 6:

  (a) each loader alone: wall time per batch up to a device synchronise behind the batch, and for the two loaders that work on
      the host where that time goes (wav read, text_to_sequence, padding, upload, front end);
  (b) each loader feeding TrainEngine.step for at least `steps` timed steps after a warm-up, with bucket_batches off and on.
      The sources take turns in blocks of `block` steps, so a drift of the machine hits all of them.  Two loops: the one of
      train.py, which reads the loss back after every step (the next batch is fetched only then), and a free-running one that
      synchronises at the end of a block;
  (c) the ceiling: the same index lists as batches that are already on the device, in the same blocks.  Every source steps an
      engine of its own, built from the same seed, so each meets the shapes a training run of its own would meet;
  (d) the share of steps that went through a captured graph (the capturing step included), the share of the eager steps that
      ran the persistent decoder kernels, and the store's build time.

Prints the table (and writes it to --out)."""
import argparse
import datetime
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron2-vae_amd'))

FRAMES_PER_SYMBOL = 389.0 / 84.0
SOURCES = ('host collate', 'device_frontend', 'resident_corpus', 'ceiling')


def write_corpus(root, n_utts, seed, n_val=30):
    """koemo-like lengths: symbols ~ lognormal(median 71, mean 84) in 5..400, frames = symbols x 4.63 x lognormal(0, 0.15)"""
    from scipy.io.wavfile import write
    from text import text_to_sequence
    rng = np.random.RandomState(seed)
    sigma = float(np.sqrt(2.0 * np.log(84.0 / 71.0)))
    lists = []
    for name, count in (('train.txt', n_utts), ('val.txt', n_val)):
        lines = []
        for i in range(count):
            symbols = int(np.clip(71.0 * np.exp(sigma * rng.randn()), 5, 400))
            text = "".join(chr(0xAC00 + int(rng.randint(0, 11172))) for _ in range(max(1, int(round(symbols / 2.96)))))
            symbols = len(text_to_sequence(text, ['korean_cleaners']))
            frames = int(np.clip(symbols * FRAMES_PER_SYMBOL * np.exp(0.15 * rng.randn()), 24, 1200))
            n = frames * 256 - int(rng.randint(1, 256))
            path = os.path.join(root, '%s_%04d.wav' % (name[:-4], i))
            write(path, 16000, (np.clip(0.1 * rng.randn(n), -1, 1) * 32767).astype(np.int16))
            lines.append("%s|%s|0|%d\n" % (path, text, int(rng.randint(0, 4))))
        lists.append(os.path.join(root, name))
        with open(lists[-1], 'w', encoding='utf-8') as f:
            f.write("".join(lines))
    return lists


class Stages(object):
    """host wall time by stage while a loader works: wrappers around the functions of the parent commit's loaders"""
    NAMES = ('wav read', 'text_to_sequence', 'front end', 'upload', 'padding')

    def __init__(self):
        self.t = dict.fromkeys(self.NAMES, 0.0)
        self._undo = []
        self._inside = 0            # seconds of front end + upload spent inside the running collate call
        self._nested = 0            # depth of nested stages: an upload made inside one belongs to that stage alone

    def _timed(self, name, fn, nested=False):
        def run(*a, **kw):
            self._nested += nested
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                dt = time.perf_counter() - t0
                self._nested -= nested
                self.t[name] += dt
                if nested:
                    self._inside += dt
        return run

    def patch(self, obj, attr, name, nested=False):
        old = getattr(obj, attr)
        setattr(obj, attr, self._timed(name, old, nested))
        self._undo.append((obj, attr, old))

    def patch_uploads(self):
        """Tensor.to(<a cuda device>) of a host tensor: the device_frontend collate's uploads"""
        old = torch.Tensor.to

        def to(t, *a, **kw):
            if self._nested or t.is_cuda or not a or not isinstance(a[0], torch.device) or a[0].type != 'cuda':
                return old(t, *a, **kw)
            t0 = time.perf_counter()
            try:
                return old(t, *a, **kw)
            finally:
                dt = time.perf_counter() - t0
                self.t['upload'] += dt
                self._inside += dt
        torch.Tensor.to = to
        self._undo.append((torch.Tensor, 'to', old))

    def wrap_collate(self, fn):
        def run(batch):
            self._inside = 0.0
            t0 = time.perf_counter()
            out = fn(batch)
            self.t['padding'] += time.perf_counter() - t0 - self._inside
            return out
        return run

    def undo(self):
        for obj, attr, old in reversed(self._undo):
            setattr(obj, attr, old)
        self._undo = []


def make_loader(hp_string, kind):
    import hparams as HP
    import train as TR
    extra = ",device_frontend=True" if kind == 'device_frontend' else ""
    hp = HP.create_hparams(hp_string + extra)
    return TR.prepare_dataloaders(hp, resident_corpus=kind == 'resident_corpus')


def cycle(loader):
    epoch = 0
    while True:
        sampler = getattr(loader, 'batch_sampler', None)
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)
        for batch in loader:
            yield batch
        epoch += 1


def index_lists(loader, n):
    """the first n index lists the loader's sampler draws (the three loaders draw the same ones: same sampler, same lengths)"""
    out, epoch = [], 0
    while len(out) < n:
        sampler = loader.batch_sampler
        if hasattr(sampler, 'set_epoch'):
            sampler.set_epoch(epoch)
        out.extend([list(b) for b in sampler])
        epoch += 1
    return out[:n]


def loaders_alone(hp_string, n_batches, emit):
    """(a): wall time per batch behind a device synchronise, and the host's stages"""
    import data_utils
    from model import BatchLayout
    emit("(a) the loaders alone: %d batches of 6, ms per batch (wall, a device synchronise behind every batch)" % n_batches)
    emit("    %-16s %8s %8s | host stages, ms per batch: %s" % ('loader', 'median', 'mean', '  '.join('%-16s' % s for s in Stages.NAMES)))
    build_s = None
    for kind in SOURCES[:3]:
        st = Stages()
        loader, _, collate_fn = make_loader(hp_string, kind)
        if kind != 'resident_corpus':
            st.patch(data_utils, 'load_wav_to_torch', 'wav read')
            st.patch(data_utils.TextMelLoader, 'get_audio', 'wav read')
            st.patch(data_utils.TextMelLoader, 'get_text', 'text_to_sequence')
            st.patch(loader.dataset.stft, 'mel_spectrogram', 'front end', nested=True)
            if kind == 'device_frontend':
                st.patch_uploads()
            loader.collate_fn = st.wrap_collate(collate_fn)
        else:
            build_s = collate_fn.corpus.build_seconds
        times = []
        try:
            it = cycle(loader)
            for i in range(n_batches + 5):
                if i == 5:
                    st.t = dict.fromkeys(Stages.NAMES, 0.0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batch = next(it)
                if kind == 'host collate':      # the batch is on the device when the step starts: the engine's staged upload
                    t1 = time.perf_counter()
                    lay = BatchLayout(batch)
                    lay.views(lay.upload(batch))
                    st.t['upload'] += time.perf_counter() - t1
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
        finally:
            st.undo()
        times = np.asarray(times[5:]) * 1e3
        stages = ('  '.join('%-16.3f' % (1e3 * st.t[s] / n_batches) for s in Stages.NAMES) if kind != 'resident_corpus'
                  else 'sort of 6 integers, one pinned upload, one launch')
        emit("    %-16s %8.3f %8.3f | %s" % (kind, float(np.median(times)), float(times.mean()), stages))
    emit("    (host collate: the front end runs per utterance inside the dataset, upload + launch + download; device_frontend: one")
    emit("     launch per batch, its uploads are the padded audio and the lengths; the rest of either collate call is `padding`)")
    return build_s


def feed_engine(hp_string, bucket, steps, block, warmup, sync_every_step, emit):
    """(b) + (c) + (d) for one setting of bucket_batches and one loop"""
    import hparams as HP
    import t2v_hip
    import train as TR
    hps = hp_string + ",bucket_batches=%s" % bucket
    hp = HP.create_hparams(hps)
    torch.manual_seed(hp.seed)
    torch.cuda.manual_seed(hp.seed)
    # one engine per source, from the same seed: every source meets the shapes it would meet in a training run of its own (an
    # engine captures a shape the third time it sees it; sources sharing one engine would capture each other's shapes)
    engines = {}
    for kind in SOURCES:
        torch.manual_seed(hp.seed)
        torch.cuda.manual_seed(hp.seed)
        engines[kind] = TR.TrainEngine(hp)
    n_blocks = -(-steps // block)
    total = warmup + n_blocks * block
    loaders = {kind: make_loader(hps, kind) for kind in SOURCES[:3]}
    corpus = loaders['resident_corpus'][2].corpus
    lists = index_lists(loaders['resident_corpus'][0], total)
    frames = [int(corpus.n_frames[b].sum()) for b in lists]
    feeds = {kind: cycle(loaders[kind][0]) for kind in SOURCES[:3]}
    stat = {k: dict(seconds=[], frames=0, steps=0, replays=0, persistent=0, eager=0) for k in SOURCES}

    def count_replays(engine, s):
        after_replay = engine._after_replay

        def counted(*a, **kw):
            s['seen'] = s.get('seen', 0) + 1
            return after_replay(*a, **kw)
        engine._after_replay = counted
    for kind in SOURCES:
        count_replays(engines[kind], stat[kind])
    ceiling = [tuple(t.clone() for t in loaders['resident_corpus'][2](b)) for b in lists]
    feeds['ceiling'] = iter(ceiling)
    torch.cuda.synchronize()
    it = 0
    for blk in range(-1, n_blocks):                 # block -1 is the warm-up of every source
        n = warmup if blk < 0 else block
        for kind in SOURCES:
            s, engine = stat[kind], engines[kind]
            with engine.stream_context():
                r0 = s.get('seen', 0)
                pers = eager = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(n):
                    seen = s.get('seen', 0)
                    out = engine.step(next(feeds[kind]), it + k)
                    if sync_every_step:
                        out[0].item()                   # train.py reads the loss back: the next batch is fetched behind it
                    if s.get('seen', 0) == seen:        # an eager step: DecoderCore's last modes are this step's (a replay leaves them stale)
                        eager += 1
                        pers += (t2v_hip.DecoderCore.last_mode == 'persistent') + (t2v_hip.DecoderCore.last_bwd_mode == 'persistent')
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            if blk >= 0:
                s['seconds'].append(dt)
                s['steps'] += n
                s['frames'] += sum(frames[warmup + blk * block:warmup + (blk + 1) * block])
                s['replays'] += s.get('seen', 0) - r0
                s['persistent'] += pers
                s['eager'] += eager
        it += n
    t2v_hip.check_async_errors()
    for engine in engines.values():
        engine.close()
    loop = "train.py's loop (loss read back every step)" if sync_every_step else "free-running (synchronise per block)"
    emit("(b, c, d) bucket_batches=%s, %s: %d timed steps per source in blocks of %d after %d warm-up steps"
         % (bucket, loop, n_blocks * block, block, warmup))
    emit("    %-16s %9s %9s %12s %10s %9s %10s" % ('source', 'ms/step', 'median', 'frames/s', 'of ceiling', 'graph hit', 'persistent'))
    emit("    (ms/step and frames/s: all timed steps; median: the median block; of ceiling: the median over the blocks of ceiling time /")
    emit("     source time for the SAME index lists, which keeps a block that holds a graph capture from deciding the ratio;")
    emit("     persistent: forward and reverse passes of the EAGER steps that took the persistent decoder kernels)")
    top = stat['ceiling']['seconds']
    res = {}
    for kind in SOURCES:
        s = stat[kind]
        ms = 1e3 * sum(s['seconds']) / s['steps']
        res[kind] = float(np.median([c / t for c, t in zip(top, s['seconds'])]))
        emit("    %-16s %9.3f %9.3f %12.0f %10.3f %8.1f%% %9.1f%%"
             % (kind, ms, 1e3 * float(np.median(s['seconds'])) / block, s['frames'] / sum(s['seconds']), res[kind],
                100.0 * s['replays'] / s['steps'], 50.0 * s['persistent'] / max(1, s['eager'])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--utts', type=int, default=600)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--block', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--alone', type=int, default=60, help='batches per loader in (a)')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    import t2v_hip
    t2v_hip.load_library()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    random.seed(args.seed)
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        train_list, val_list = write_corpus(root, args.utts, args.seed)
        emit("Data path of train.py: %s (%s), %s, torch %s, %d host threads; seed %d, %d utterances written in %.1f s"
             % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName.split(':')[0],
                datetime.date.today().isoformat(), torch.__version__, torch.get_num_threads(),
                args.seed, args.utts, time.perf_counter() - t0))
        hp_string = "batch_size=6,anneal_function=constant,training_files=%s,validation_files=%s" % (train_list, val_list)
        build_s = loaders_alone(hp_string, args.alone, emit)
        emit("(d) the resident corpus of %d + 30 utterances was built in %.2f s (host tables and device store)" % (args.utts, build_s))
        emit()
        for sync in (True, False):
            for bucket in (False, True):
                feed_engine(hp_string, bucket, args.steps, args.block, args.warmup, sync, emit)
                emit()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
