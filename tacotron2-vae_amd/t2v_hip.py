"""ctypes binding of libt2vae_hip.so (C ABI in include/t2vae.h) + the autograd wrappers
the boundary modules in model.py call.

There is no CPU fallback: every op raises `T2VHipError` when the shared library or a GPU
is missing, so a silent eager path can never stand in for the HIP kernels.
"""
import collections
import ctypes as C
import math
import operator
import os

import torch

import t2v_abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (T2V_LIB: another build of the same library — A/B measurements of two kernel variants on ONE GPU box, tools/dbg/ab_lib.sh)
_LIB_PATH = os.environ.get('T2V_LIB') or os.path.join(_HERE, 'libt2vae_hip.so')
_lib = None

H, E, PRE, A, F_LOC, KS, XW, KATT, KATT_INF, G4 = 1024, 512, 256, 128, 32, 31, 2560, 1536, 1792, 4096

# The C ABI comes from include/t2vae.h itself (t2v_abi.py parses it once per process): the entry points with their
# argument / return types, the struct layouts and the integer limits.  Nothing of it is restated here, so a new entry
# point is declared in the header and needs no line in this file.
_ABI = t2v_abi.load()
T2VHipError = t2v_abi.T2VHipError

# the ctypes.Structure of every struct the host fills (pointer fields are c_void_p; C_NAME is the C struct's name)
(_DecWeights, _DecTrainBufs, _DecBwdBufs, _DecPersistWeights, _DecPersistBufs, _DecTrainPersistWeights, _GemmGroup, _AchainDw,
 _DecInferBufs, _DecItems, _DecWindow) = (_ABI.classes[n] for n in (
     't2v_dec_weights', 't2v_dec_train_bufs', 't2v_dec_bwd_bufs', 't2v_dec_persist_weights', 't2v_dec_persist_bufs',
     't2v_dec_train_persist_weights', 't2v_gemm_group', 't2v_achain_dw', 't2v_dec_infer_bufs', 't2v_dec_items', 't2v_dec_window'))
_StepRecord = _ABI.classes['t2v_step_params']       # lives in device memory: only its layout is used here (StepParams)
if (_StepRecord.epoch.offset, _StepRecord.epoch.size) != (0, 8):        # StepParams.upload() writes it as a slot's first int64
    raise T2VHipError("t2v_step_params.epoch is not the 8-byte field at offset 0 (include/t2vae.h)")

EXPORTS = tuple(_ABI.prototypes)


def lib_path():
    return _LIB_PATH


def load_library():
    """dlopen the in-tree library (no compute) and give every entry point of the header its types; raises T2VHipError when
    the library is not built, AttributeError when it lacks a declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(_LIB_PATH):
        raise T2VHipError("libt2vae_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C tacotron2-vae_amd/csrc)")
    lib = C.CDLL(_LIB_PATH)
    for name, (restype, argtypes) in _ABI.prototypes.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = lib
    return lib


# ---- precision switch (hparams.bf16_run, BASELINE configs[4]).  Off: everything is fp32.  On: the k=5 Conv1d
# forward / data-gradient kernels, the time-batched linear layers (own GEMM) and the deferred LSTM weight-gradient
# GEMMs (library) take bf16 operands with fp32 accumulation; master weights, BatchNorm, the recurrent state, the
# per-step LSTM / attention kernels, loss and Adam stay fp32.
_BF16 = False

# BatchNorm `num_batches_tracked` counters touched by the current forward pass: bumped together by ONE
# multi-tensor launch (flush_bn_counters) instead of one tiny kernel per layer (14 per step)
_BN_PENDING = []


def note_bn_counter(t):
    _BN_PENDING.append(t)


_BN_DEFER = [0]


def flush_bn_counters():
    if _BN_PENDING and not _BN_DEFER[0]:
        torch._foreach_add_(_BN_PENDING, 1)
        del _BN_PENDING[:]


class defer_bn_counters(object):
    """inside this context the per-module flushes are postponed: the whole model's counters (14 BatchNorm layers) are
    bumped by one launch when the outermost context exits"""

    def __enter__(self):
        _BN_DEFER[0] += 1

    def __exit__(self, *exc):
        _BN_DEFER[0] -= 1
        if exc[0] is None:
            flush_bn_counters()
        elif not _BN_DEFER[0]:
            del _BN_PENDING[:]
        return False


def set_bf16(on):
    global _BF16
    _BF16 = bool(on)


def bf16_enabled():
    return _BF16


# ---- per-step parameters in device memory (include/t2vae.h: t2v_step_params).  Kernel arguments are frozen when the
# training step is captured into a HIP graph; the kernels read this 32-byte record at run time instead (dropout epoch,
# Adam lr / bias corrections, KL weight).  Host values go through a ring of pinned slots: the H2D copy is asynchronous
# and the host runs ahead of the GPU, so a slot must not be rewritten before its copy has executed.
_DEFAULT_REC = [None]      # the StepParams currently installed as the process default (stream=None records)


class StepParams(object):
    """One engine's record.  stream=None: installed as the process default (read by launches on any stream that has no
    binding of its own); stream=<torch.cuda.Stream>: bound to that stream only (t2v_set_step_params_stream), so two engines
    in one process never share a record."""
    RING = 256
    WORDS = C.sizeof(_StepRecord) // 4       # the record as 4-byte words: the 8-byte epoch, then fp32 slots
    SLOTS = {n: getattr(_StepRecord, n).offset // 4 for n, t in _StepRecord._fields_ if t is C.c_float}

    def __init__(self, device, stream=None):
        lib = load_library()
        self.host = torch.zeros(self.RING, self.WORDS, dtype=torch.float32).pin_memory()
        self.dev = torch.zeros(self.WORDS, dtype=torch.float32, device=device)
        self.cur = dict(epoch=0, lr=0.0, bc1=1.0, bc2s=1.0, kl_weight=0.0)
        self.dirty = True
        self._i = 0
        self.stream = stream
        self.extra_streams = []      # the engine's side streams (Overlap): kernels launched there read the same record
        if stream is None:
            lib.t2v_set_step_params(C.c_void_p(self.dev.data_ptr()))
            _DEFAULT_REC[0] = self
        else:
            self.bind()

    def bind(self, extra=None):
        """(re)bind this record to its stream(s).  torch hands out pooled native streams round-robin, so a later engine
        may have taken over a handle: the engine whose step is being issued re-binds before it launches"""
        if extra is not None:
            self.extra_streams = list(extra)
        if self.stream is None:
            return
        lib = load_library()
        for st in [self.stream] + self.extra_streams:
            _check(lib.t2v_set_step_params_stream(C.c_void_p(st.cuda_stream), C.c_void_p(self.dev.data_ptr())),
                   't2v_set_step_params_stream')

    def set(self, **kw):
        for k, v in kw.items():
            v = int(v) if k == 'epoch' else float(v)
            if self.cur[k] != v:
                self.cur[k] = v
                self.dirty = True

    def upload(self, force=False):
        """enqueue the record on the current stream if it changed (never inside a graph capture: the training engine
        sets every field before it captures or replays)"""
        if not (self.dirty or force):
            return
        if torch.cuda.is_current_stream_capturing():
            raise T2VHipError("step parameters changed inside a graph capture")
        slot = self.host[self._i % self.RING]
        self._i += 1
        slot.view(torch.int64)[0] = self.cur['epoch']
        for k, i in self.SLOTS.items():
            slot[i] = self.cur[k]
        self.dev.copy_(slot, non_blocking=True)
        self.dirty = False

    def release(self):
        lib = load_library()
        if self.stream is None:
            if _DEFAULT_REC[0] is self:         # a later engine may have installed ITS record as the process default
                lib.t2v_set_step_params(None)
                _DEFAULT_REC[0] = None
        else:
            for st in [self.stream] + self.extra_streams:
                lib.t2v_set_step_params_stream(C.c_void_p(st.cuda_stream), None)


_STEP = None          # the ACTIVE record: the one of the engine whose step is being issued (or the process default)
_STEP_ALL = []


# ---- explicit multi-stream choreography of a training step (round 4).  A step is a handful of long dependent chains
# (encoder conv bank -> BiLSTM, reference encoder, Prenet -> gpre, Postnet data gradients, BiLSTM BPTT ...) made of
# latency-bound kernels that fill a fraction of the 256 CUs, plus bulk work nothing downstream waits for (every weight
# gradient).  `Overlap` owns the side streams of ONE training engine: `side(name)` forks a named stream off the current
# one (the side stream waits for everything issued so far on the current stream, later launches on the two run
# concurrently); `join()` makes the current stream wait for every side stream used since the last join and is called by
# the engine before gradients are consumed (all-reduce / clip + Adam).  Under graph capture the forks and joins become
# graph edges.  Tensors that were allocated on the forking stream and are read on a side stream are kept alive until the
# join (`keep=`), so the caching allocator cannot hand their memory to a later main-stream launch while the side stream
# still reads it.  With no engine active (`overlap() is None`, e.g. a bare `model(x)` + `loss.backward()`), `side()`
# runs its body inline on the current stream: nothing changes for code outside the training engine.
class Overlap(object):
    # reference-encoder branch; deferred ("nobody waits for it") work: weight gradients, Prenet; the four chip-filling LSTM
    # weight-gradient GEMMs of the decoder get a stream of their own so the long tail of small deferred kernels runs next to them
    # 'd': idle — the step has no work for it any more; it stays so that every stream created after these keeps its pooled handle
    NAMES = ('vae', 'w', 'g', 'd')

    def __init__(self, device=None):
        self.on = True
        # (T2V_MAIN_PRIO / T2V_SIDE_PRIO, measurement: stream priorities of the engine's own stream and of the side streams —
        # three same-box pairs showed no difference)
        lo = int(os.environ.get('T2V_SIDE_PRIO', '0'))
        self._streams = {n: torch.cuda.Stream(device=device, priority=lo) for n in self.NAMES}
        self._used = []
        self._keep = []

    def streams(self):
        return list(self._streams.values())

    def stream(self, name):
        return self._streams[name]

    class _Inline(object):
        def __enter__(self):
            return False

        def __exit__(self, *exc):
            return False

    class _Fork(object):
        def __init__(self, st):
            self.ctx = torch.cuda.stream(st)

        def __enter__(self):
            self.ctx.__enter__()
            return True

        def __exit__(self, *exc):
            return self.ctx.__exit__(*exc)

    def mark(self):
        """an event on the current stream: `side(..., after=mark)` forks from THAT point even when the fork is issued later
        (the host issues the critical chain first, the side chains still start where the mark was taken)"""
        if not self.on:
            return None
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def side(self, name, keep=(), after=None):
        """`with ov.side('w', keep=(dy, x)) as forked:` — body runs on the named side stream (forked=True) or inline"""
        if not self.on:
            return Overlap._Inline()
        st = self._streams[name]
        cur = torch.cuda.current_stream()
        if cur == st:
            return Overlap._Inline()
        if after is not None:
            st.wait_event(after)
        else:
            st.wait_stream(cur)
        self._keep.extend(t for t in keep if t is not None)
        if st not in self._used:
            self._used.append(st)
        return Overlap._Fork(st)

    def wait(self, name):
        """the current stream waits for what has been issued on one side stream so far (a mid-step hand-over; the
        stream stays registered for the final join)"""
        st = self._streams[name]
        if self.on and st in self._used and torch.cuda.current_stream() != st:
            torch.cuda.current_stream().wait_stream(st)

    def join(self):
        cur = torch.cuda.current_stream()
        if _STAMPS['on']:
            for n, st in self._streams.items():
                if st in self._used and st != cur:
                    with torch.cuda.stream(st):
                        stamp('side_%s_end' % n)
        for st in self._used:
            if st != cur:
                cur.wait_stream(st)
        self._used = []
        self._keep = []
        _PREFLIP.clear()        # flipped conv weights belong to the step that made them
        BiLSTM._prep.clear()
        flush_err_notes()       # every stream that wrote an error word has been joined: one gather launch for the step


# ---- phase stamps (T2V_STAMPS=1): one-thread launches that write the 100 MHz wall clock at named points of the step
_STAMPS = {'on': os.environ.get('T2V_STAMPS', '0') == '1', 'buf': None, 'names': []}


def stamp(name):
    """drop a time stamp into the current stream (no-op unless T2V_STAMPS=1); tools/stamps.py reads them back"""
    if not _STAMPS['on']:
        return
    only = os.environ.get('T2V_STAMP_ONLY')
    if only and name not in only.split(','):
        return
    if _STAMPS['buf'] is None:
        _STAMPS['buf'] = torch.zeros(256, dtype=torch.int64, device='cuda')
    if name not in _STAMPS['names']:
        _STAMPS['names'].append(name)
    slot = _STAMPS['names'].index(name)
    _check(load_library().t2v_stamp(C.c_void_p(_STAMPS['buf'].data_ptr()), slot, _stream()), 't2v_stamp')


def read_stamps():
    """{name: microseconds since the earliest stamp} of the last executed step (synchronises)"""
    if _STAMPS['buf'] is None:
        return {}
    torch.cuda.synchronize()
    v = _STAMPS['buf'][:len(_STAMPS['names'])].cpu().tolist()
    t0 = min(v)
    return {n: (x - t0) / 100.0 for n, x in zip(_STAMPS['names'], v)}


_OVERLAP = [None]


def overlap():
    """the Overlap manager of the engine whose step is being issued, else None"""
    return _OVERLAP[0]


def set_overlap(ov):
    prev = _OVERLAP[0]
    _OVERLAP[0] = ov
    return prev


def side(name, keep=(), after=None):
    """fork onto a side stream of the active engine, or run inline when no engine is active / overlap is off"""
    ov = _OVERLAP[0]
    return ov.side(name, keep, after) if ov is not None else Overlap._Inline()


def mark():
    ov = _OVERLAP[0]
    return ov.mark() if ov is not None else None


def step_params(create=True, stream=None, fresh=False):
    """the active StepParams (None until a training engine asks for one with create=True).  fresh=True: a new record for
    a new engine (bound to `stream` when given); it becomes the active one."""
    global _STEP
    if (_STEP is None and create) or fresh:
        _STEP = StepParams(torch.device('cuda', torch.cuda.current_device()), stream=stream)
        _STEP_ALL.append(_STEP)
    return _STEP


def activate_step_params(sp):
    """an engine calls this at the top of every step: the Python-side helpers (FlatAdam.step, VAELoss, the model's
    per-forward dropout counters) then talk to THIS engine's record.  A record that is not bound to a stream is also
    (re)installed as the process default."""
    global _STEP
    if sp is not None and sp.stream is not None:
        sp.bind()       # every step: another engine (dead or alive) may have taken or dropped the pooled stream handle
    if _STEP is not sp:
        _STEP = sp
    if sp is not None and sp.stream is None and _DEFAULT_REC[0] is not sp:
        load_library().t2v_set_step_params(C.c_void_p(sp.dev.data_ptr()))
        _DEFAULT_REC[0] = sp


def drop_step_params(sp):
    """an engine that is closed / garbage-collected unbinds its record (captured graphs keep the memory alive)"""
    global _STEP
    if sp in _STEP_ALL:
        _STEP_ALL.remove(sp)
        try:
            sp.release()
        except Exception:
            pass
    if _STEP is sp:
        _STEP = None


def release_step_params():
    """uninstall every device record (the kernels fall back to their by-value arguments); engines created later install
    new ones.  Captured graphs of an engine keep reading the old record's memory, which stays allocated with them."""
    global _STEP
    for sp in _STEP_ALL:
        sp.release()
    del _STEP_ALL[:]
    if _STEP is not None:
        load_library().t2v_set_step_params(None)
        _STEP = None
    _DEFAULT_REC[0] = None


# ---- asynchronous error ledger.  The cooperative kernels (BiLSTM, GRU, attention exchange, reverse-step hand-off)
# use bounded spins: on a timeout they set an error word and leave instead of hanging.  Reading those words right
# away would force a device sync per call, so the wrappers copy each word (device-to-device, 4 bytes) into a small
# per-device ledger and `check_async_errors()` — called by the training loop where it syncs anyway (loss.item()),
# by validate(), bench.py and the tests — reads the ledger once and raises if any call reported a timeout.
#
# Layout of the ledger (round 5): two regions.
#   [0, _ERR_GRAPH_SLOTS)            blocks of _ERR_BLOCK slots, one block per CAPTURED graph.  The gather launches of a
#                                    captured step write their words into the graph's own block on every replay, so the block
#                                    stays reserved while the graph lives and goes back to the free list when the graph is
#                                    evicted (err_capture_begin / err_capture_end / err_release).  A training engine reads
#                                    `err_words(span)` of the graph it just replayed: that is the guard of the optimiser step.
#   [_ERR_GRAPH_SLOTS, _ERR_SLOTS)   eager notes.  A step reserves a contiguous run (err_mark: when fewer than
#                                    _ERR_STEP_RESERVE slots are left the ledger is checked — a sync, and a raise if a word
#                                    is set — and the cursor goes back to the start of the region), so err_range(mark) never
#                                    spans a wrap and no slot index ever reaches _ERR_SLOTS.
_ERR_POOL = {}
_ERR_SLOTS = 4096
_ERR_BLOCK = 32             # ledger words of one captured graph (a step has six or seven cooperative launches)
_ERR_GRAPH_SLOTS = 2048     # 64 captured graphs alive at once, over all engines of the process
_ERR_STEP_RESERVE = 64


# test hook: a substring — the next ledger entry whose label contains it is recorded as a time-out — or (substring, label): the
# entry is recorded as a time-out under that label (two ranks sharing one GPU cannot run the persistent kernels, but the
# recovery path keys on their label)
_ERR_INJECT = [None]


class _ErrPool(object):
    def __init__(self, device):
        self.words = torch.zeros(_ERR_SLOTS, device=device, dtype=torch.int32)
        self.cursor = _ERR_GRAPH_SLOTS          # next eager slot
        self.labels = {}
        self.free_blocks = list(range(0, _ERR_GRAPH_SLOTS, _ERR_BLOCK))
        self.capture = None                     # [lo, next, hi] of the block the running capture writes
        self.used_hi = _ERR_GRAPH_SLOTS         # eager slots [GRAPH_SLOTS, used_hi) may hold unchecked words


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _err_pool(device=None):
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    key = str(dev)
    pool = _ERR_POOL.get(key)
    if pool is None:
        pool = _ERR_POOL[key] = _ErrPool(dev)
    return key, pool


def _err_take_slot(pool):
    if pool.capture is not None:
        lo, nxt, hi = pool.capture
        if nxt >= hi:
            raise T2VHipError("more than %d cooperative launches inside one captured graph" % _ERR_BLOCK)
        pool.capture[1] = nxt + 1
        return nxt
    if pool.cursor >= _ERR_SLOTS:
        # a loop that never checks its errors: check now (syncs; raises if a kernel timed out), then start over
        if _capturing():
            raise T2VHipError("error ledger full inside a graph capture that did not reserve a block")
        check_async_errors()
    slot = pool.cursor
    pool.cursor += 1
    pool.used_hi = max(pool.used_hi, pool.cursor)
    return slot


def _err_note(label, word):
    """word: a 1-element int32 device view holding a kernel's error word (valid once the stream reaches it)"""
    key, pool = _err_pool(word.device)
    slot = _err_take_slot(pool)
    assert 0 <= slot < _ERR_SLOTS
    # (round 4) the 4-byte copy into the ledger is deferred: flush_err_notes() moves up to 16 words per launch (a step has
    # six or seven cooperative launches; each copy was a launch of its own on the critical path)
    want = _ERR_INJECT[0]
    inject = want is not None and (want if isinstance(want, str) else want[0]) in label
    if inject:
        if not isinstance(want, str):
            label = want[1]
        _ERR_INJECT[0] = None
    _ERR_PENDING.setdefault(key, []).append((slot, word, torch.cuda.current_stream(word.device), inject))
    pool.labels[slot] = label
    if len(_ERR_PENDING[key]) >= 16:
        flush_err_notes()


_ERR_PENDING = {}


def flush_err_notes():
    """copy the pending error words into the ledger with one launch per 16 words, on the current stream (which first waits
    for any other stream a pending word was written on).  The training engine calls it where its side streams have joined;
    check_async_errors() calls it before it reads the ledger."""
    for key, pend in list(_ERR_PENDING.items()):
        if not pend:
            continue
        pool = _ERR_POOL[key]
        dev = pool.words.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            for st in {id(p[2]): p[2] for p in pend if p[2] != cur}.values():
                cur.wait_stream(st)
            n = len(pend)
            src = (C.c_void_p * n)(*[p[1].data_ptr() for p in pend])
            dst = (C.c_void_p * n)(*[pool.words.data_ptr() + 4 * p[0] for p in pend])
            _check(load_library().t2v_gather_words(src, dst, n, _stream()), 't2v_gather_words')
            for p in pend:
                p[1].record_stream(cur)
                if p[3]:
                    pool.words[p[0]:p[0] + 1].fill_(1)
        del pend[:]


def err_mark(device=None):
    """position of the error ledger now: an engine takes it at the top of a step; err_range(mark) then names the ledger words
    the step's kernels wrote (the guard of the fused optimiser step).  Reserves a contiguous run for the step: with fewer
    than _ERR_STEP_RESERVE eager slots left the ledger is checked (sync; raises on a recorded time-out) and restarted."""
    _, pool = _err_pool(device)
    if pool.capture is not None:
        return pool.capture[1]
    if pool.cursor + _ERR_STEP_RESERVE > _ERR_SLOTS and not _capturing():
        check_async_errors()
    return pool.cursor


def err_range(mark, device=None):
    """int32 device view of the ledger words written since `mark` (None when there are none)"""
    _, pool = _err_pool(device)
    cur = pool.capture[1] if pool.capture is not None else pool.cursor
    if cur <= mark:
        return None
    return pool.words[mark:cur]


def err_words(span, device=None):
    """int32 device view of the ledger block (lo, hi) of a captured graph (None for an empty block)"""
    if span is None or span[1] <= span[0]:
        return None
    _, pool = _err_pool(device)
    return pool.words[span[0]:span[1]]


def err_capture_begin(device=None):
    """right before a graph capture: reserve a ledger block for the graph.  The notes of the capture land in it (and every
    replay rewrites them there).  Returns False when no block is free — the caller then does not capture (the step runs
    eagerly), instead of pinning ledger slots without bound."""
    _, pool = _err_pool(device)
    if pool.capture is not None:
        raise T2VHipError("nested graph captures share no error-ledger block")
    flush_err_notes()               # eager notes still pending must not be swept into the captured gather
    if not pool.free_blocks:
        return False
    lo = pool.free_blocks.pop(0)
    pool.capture = [lo, lo, lo + _ERR_BLOCK]
    return True


def err_capture_end(device=None, keep=True):
    """after the capture: (lo, hi) of the words the graph writes on every replay; keep=False (capture failed) frees the block"""
    key, pool = _err_pool(device)
    if pool.capture is None:
        return None
    lo, nxt, _hi = pool.capture
    pool.capture = None
    if _ERR_PENDING.get(key):       # notes of a capture that died before its flush: their words never get written
        _ERR_PENDING[key] = [p for p in _ERR_PENDING[key] if not (lo <= p[0] < lo + _ERR_BLOCK)]
    if not keep:
        err_release((lo, nxt), device)
        return None
    return (lo, nxt)


def err_release(span, device=None):
    """the graph that owned ledger block `span` is gone: labels dropped, block back on the free list"""
    if span is None:
        return
    _, pool = _err_pool(device)
    lo = span[0] - span[0] % _ERR_BLOCK
    for i in range(lo, lo + _ERR_BLOCK):
        pool.labels.pop(i, None)
    if lo not in pool.free_blocks and 0 <= lo < _ERR_GRAPH_SLOTS:
        pool.words[lo:lo + _ERR_BLOCK].zero_()
        pool.free_blocks.append(lo)
        pool.free_blocks.sort()


def check_async_errors():
    """Raise T2VHipError if any cooperative kernel since the last check reported a barrier timeout (syncs)."""
    bad = []
    flush_err_notes()
    for key, pool in _ERR_POOL.items():
        n = max(pool.used_hi, pool.cursor)
        vals = pool.words[:n].cpu()
        for i in torch.nonzero(vals).flatten().tolist():
            bad.append(pool.labels.get(i, '?'))
        pool.words[:n].zero_()
        pool.cursor = pool.used_hi = _ERR_GRAPH_SLOTS
        for i in [i for i in pool.labels if i >= _ERR_GRAPH_SLOTS]:
            del pool.labels[i]
    if bad:
        e = T2VHipError("cooperative kernel barrier timed out (results of that step are invalid): %s"
                        % ", ".join(sorted(set(bad))))
        e.labels = sorted(set(bad))
        raise e


def _require_gpu(*tensors):
    lib = load_library()
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise T2VHipError("HIP op called with a CPU tensor; this path has no CPU fallback")
    return lib


def _check(rc, what):
    if rc != 0:
        raise T2VHipError("%s failed: rc=%d (%s)" % (what, rc, load_library().t2v_last_error().decode()))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    assert t.dtype == torch.float32
    return t.contiguous()


MAX_DEC_B = 16      # batch columns of one MFMA tile in the per-step kernels; larger batches run in chunks

# ---- the kernel sets of the teacher-forced decoder.  DecoderCore.plan() picks one forward and one reverse engine per batch
# chunk; _fwd_chunk(), backward() and the replay_* functions read the engine's record and never choose themselves.
# Library entry points are held by name.  The launch-per-step pair ('steps') has no record: it is the general path.
_FwdEngine = collections.namedtuple('_FwdEngine', 'kernel scratch run')
_FWD_ENGINES = {
    'persist': _FwdEngine('k_dec_train_persist', 't2v_decoder_train_persist_scratch_floats', 't2v_decoder_train_fwd_persistent'),
    'persist16': _FwdEngine('k_dec_train_persist16', 't2v_decoder_train_persist16_scratch_floats',
                            't2v_decoder_train_fwd_persistent16'),
}
# slices / scratch / dq_offset: size queries.  dq_rows: row stride of the (T, rows, 128) view of dq(t) inside scratch (None = the
# chunk's batch).  prepare / prepared / run: the preparation alone, the pass behind it, both in one call.  arena_prepare: the
# preparation reads the forward arena (its factor arrays) and takes the dropout arguments; reserved: prepared / run take the
# header's `dw` pointer (weight-gradient epilogue, None = none) behind the weights.  keep: arena tensors the preparation reads on the deferred-work stream.
_BwdEngine = collections.namedtuple('_BwdEngine', 'kernel slices scratch dq_offset dq_rows prepare prepared run arena_prepare '
                                                  'reserved keep')
_BWD_ENGINES = {
    'achain': _BwdEngine('k_achain_bwd', 't2v_decoder_bwd_persist_slices', 't2v_decoder_bwd_achain_scratch_floats',
                         't2v_decoder_bwd_achain_dq_offset', None, 't2v_decoder_bwd_achain_prepare',
                         't2v_decoder_bwd_achain_prepared', 't2v_decoder_bwd_achain', True, True, ('XS', 'CA', 'CD', 'GA', 'GD')),
    'persist16': _BwdEngine('k_bwd_persist16', 't2v_decoder_bwd_persist16_slices', 't2v_decoder_bwd_persist16_scratch_floats',
                            't2v_decoder_bwd_persist16_dq_offset', 16, 't2v_decoder_bwd_persistent16_prepare',
                            't2v_decoder_bwd_persistent16_prepared', 't2v_decoder_bwd_persistent16', False, False, ('XS',)),
}
_STEPS_KERNELS = {'fwd': 'k_lstm_fwd256 + k_attn_fwd', 'bwd': 'k_lstm_bwd256 + k_attn_cell_bwd'}
# the forward arena of a chunk, in the order DecoderCore keeps it (last_call[3], ctx.chunks): the fields of t2v_dec_train_bufs
_ARENA = tuple(n for n, _ in _DecTrainBufs._fields_)
# one batch chunk [b0, b1): fwd 'persist' | 'persist16' | 'steps'; bwd 'achain' | 'persist16' | 'steps' | None (no gradient);
# prepare: the reverse pass's preparation is issued right behind the forward launch; dw_epilogue: the decoder_rnn workgroups of
# the fp32 one-launch reverse pass work on decoder_rnn's weight gradients once their chain has ended (t2v_achain_dw)
ChunkPlan = collections.namedtuple('ChunkPlan', 'b0 b1 fwd bwd prepare dw_epilogue')


def _chunk_seed(seed, b0):
    """dropout seed of the batch chunk that starts at item b0 (the same in the forward and the reverse pass)"""
    return (int(seed) + 7919 * b0) & 0x7FFFFFFFFFFFFFFF


def _cat(parts, dim):       # the chunks' tensors as one: torch.cat, without the copy when there is one chunk
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim)


def _persist_weights(raw, bias_dec, wcomb, vv):
    w_ih_att, w_hh_att, w_ih_dec, w_hh_dec, wq = raw
    return _DecTrainPersistWeights(_p(w_ih_att), _p(w_hh_att), _p(w_ih_dec), _p(w_hh_dec), _p(bias_dec), _p(wq), _p(wcomb), _p(vv))


def _bwd_launch(lib, eng, prepared, PW, Sb, bufs, dims, dw=None, dal=None):
    """one-launch reverse pass of engine `eng`: bufs = (dHC, DGA, DGD, DCTX, DV, DQP, scratch, err_word),
    dims = (B, T_in, T, p_att, p_dec, seed); prepared: the preparation has been issued on these buffers;
    dw: the _AchainDw of the weight-gradient epilogue ('achain' only: the slot behind the weights);
    dal: the alignment gradient, contiguous (T, B, T_in) — the entry point's *_align sibling takes it behind dHC"""
    name = eng.prepared if prepared else eng.run
    assert dw is None or eng.reserved
    head = (C.byref(PW), None if dw is None else C.byref(dw), C.byref(Sb)) if eng.reserved else (C.byref(PW), C.byref(Sb))
    ptrs = tuple(_p(t) for t in bufs)
    if dal is not None:
        name, ptrs = name + '_align', ptrs[:1] + (_p(dal),) + ptrs[1:]
    _check(getattr(lib, name)(*(head + ptrs + tuple(dims) + (_stream(),))), name)


def replay_fwd_kernels(kernel_mask):
    """Re-issue the k_lstm_fwd256 (mask 1) / k_attn_fwd (mask 2) launches of the most recent DecoderCore.forward
    (first batch chunk) on its saved arena (bench.py roofline leg; needs DecoderCore.keep_last = True)."""
    if DecoderCore.last_call is None:
        raise T2VHipError("replay_fwd_kernels: set DecoderCore.keep_last = True before the forward pass")
    W, Sb, (B, T_in, T, p_att, p_dec, seed), _keep = DecoderCore.last_call
    _check(load_library().t2v_decoder_replay_fwd_kernels(C.byref(W), C.byref(Sb), B, T_in, T, p_att, p_dec,
                                                         seed, int(kernel_mask), _stream()),
           't2v_decoder_replay_fwd_kernels')
    return T + 1 if kernel_mask == 1 else T


def replay_persistent_forward():
    """Re-issue the persistent forward launch (csrc/decoder_train_persist.hip) of the most recent DecoderCore.forward on
    its arena — timing only (bench.py roofline leg; needs DecoderCore.keep_last = True).  Returns the launches issued (1)."""
    if DecoderCore.last_persist is None:
        raise T2VHipError("replay_persistent_forward: the last forward pass did not run on the persistent kernel (or "
                          "DecoderCore.keep_last was off)")
    PW, Sb, scratch, dims, _keep = DecoderCore.last_persist
    eng = _FWD_ENGINES[DecoderCore.last_persist_engine]
    _check(getattr(load_library(), eng.run)(C.byref(PW), C.byref(Sb), _p(scratch), *(tuple(dims) + (_stream(),))), eng.run)
    return 1


def replay_persistent_backward():
    """Re-issue the one-launch persistent reverse pass (csrc/decoder_train_bwd_persist.hip) of the most recent
    DecoderCore.backward on its buffers — timing only (S already holds dpre: the numbers it produces are not used)."""
    if DecoderCore.last_bwd_persist is None:
        raise T2VHipError("replay_persistent_backward: the last backward pass did not run on the persistent kernel (or "
                          "DecoderCore.keep_last was off)")
    PW, Sb, bufs, dims, _keep = DecoderCore.last_bwd_persist
    # (with the weight-gradient epilogue when the pass had one: the call's own preparation zeroes its control words, the tiles it
    # takes are computed again)
    dwh = _keep[-1] if isinstance(_keep[-1], GroupedHandOver) else None
    _bwd_launch(load_library(), _BWD_ENGINES[DecoderCore.last_bwd_persist_engine], False, PW, Sb, bufs, dims, None if dwh is None else dwh.dw)
    return 1


def replay_bwd_kernels(kernel_mask):
    """Re-issue the k_lstm_bwd256 (mask 1) / k_attn_cell_bwd (mask 2) launches of the most recent DecoderCore.backward
    (first batch chunk) on its buffers — timing only (bench.py roofline leg; needs DecoderCore.keep_last = True)."""
    if DecoderCore.last_bwd is None:
        raise T2VHipError("replay_bwd_kernels: no backward pass was kept (DecoderCore.keep_last = True before the step)")
    W, Sb, Gb, (B, T_in, T, p_att, p_dec, seed), _keep = DecoderCore.last_bwd
    _check(load_library().t2v_decoder_replay_bwd_kernels(C.byref(W), C.byref(Sb), C.byref(Gb), B, T_in, T, p_att, p_dec,
                                                         seed, int(kernel_mask), _stream()),
           't2v_decoder_replay_bwd_kernels')
    return T if kernel_mask == 1 else T + 1


def pack_decoder_weights(w_ih_att, w_hh_att, w_ih_dec, w_hh_dec, k_att, need_bwd, bf16=False, need_fwd=True):
    """MFMA-fragment tiles of the two decoder LSTM cells, read straight from the nn.LSTMCell tensors.  bf16=True
    (bf16_run, training pass): the same tiles rounded to bf16 — the per-step kernels stream half the bytes."""
    lib = load_library()
    dev = w_ih_att.device
    f32 = dict(device=dev, dtype=torch.float32)
    w_ih_att, w_hh_att, w_ih_dec, w_hh_dec = (_f32c(t.detach()) for t in (w_ih_att, w_hh_att, w_ih_dec, w_hh_dec))
    need_fwd = need_fwd or not need_bwd
    packF_att = torch.empty(G4 * k_att, **f32) if need_fwd else None
    packF_dec = torch.empty(G4 * XW, **f32) if need_fwd else None
    packB_att = torch.empty(G4 * KATT, **f32) if need_bwd else None
    packB_dec = torch.empty(G4 * XW, **f32) if need_bwd else None
    fn = lib.t2v_pack_lstm_weights_bf16 if bf16 else lib.t2v_pack_lstm_weights
    _check(fn(_p(w_ih_att), _p(w_hh_att), _p(w_ih_dec), _p(w_hh_dec), int(k_att),
              _p(packF_att), _p(packF_dec), _p(packB_att), _p(packB_dec), _stream()), 't2v_pack_lstm_weights')
    return packF_att, packF_dec, packB_att, packB_dec


def fuse_location_weights(loc_conv, loc_dense):
    """Fused filter bank of LocationLayer (conv then dense, both bias-free: one linear map), W_comb (128,64) stored
    twice in the orders the forward / backward kernels read it: [0] = F[d][g][st] = W_comb[d][4st+g],
    [1] viewed (64,4,32) = R[kk][g][st] = W_comb[4st+g][kk]."""
    lib = load_library()
    wcomb = torch.empty(2, A, 64, device=loc_conv.device, dtype=torch.float32)
    _check(lib.t2v_fuse_location_weights(_p(loc_conv), _p(loc_dense), _p(wcomb), _stream()), 't2v_fuse_location_weights')
    return wcomb


class DecoderCore(torch.autograd.Function):
    """Teacher-forced decoder recurrence (reference Decoder.forward loop, model.py:415-421).

    inputs : gpre (T,B,4096), memory (B,T_in,512), pm (B,T_in,128), lengths int32 (B) | None,
             attention_rnn weight_ih/weight_hh, decoder_rnn weight_ih/weight_hh, bias_dec (4096),
             query weight (128,1024), location conv (32,2,31), location dense (128,32), v (1,128)
    outputs: HC (T,B,1536) = [h_dec_t | ctx_t],  alignments (B,T,T_in)
    Both outputs are differentiable: a gradient of the alignments (a loss that reads the attention, GuidedAttention) enters the
    softmax backward of every step inside the reverse kernels; an output the loss does not use arrives as None and costs nothing.
    Batches larger than 16 run as independent chunks of <= 16 items (the loop has no cross-item coupling), so the
    reference's default batch_size = 64 works; weight gradients are summed over the chunks.
    forward() asks plan() once which kernels every chunk runs on and carries the answer on the autograd context.
    """
    # ---- switches (read by plan() alone)
    # T2V_TRAIN_PERSISTENT=0 forces the launch-per-step forward; the default takes the one-launch persistent kernel
    # (csrc/decoder_train_persist.hip) whenever t2v_decoder_train_persist_supported(B, T_in): B <= 6, T_in <= 560
    persistent = None
    persistent_bwd = None   # same switch for the reverse pass (env T2V_BWD_PERSISTENT, default: as T2V_TRAIN_PERSISTENT)
    # round 5: under bf16_run, batches of 7..16 items take the MFMA-batched persistent forward (csrc/decoder_train_persist16.hip:
    # bf16 weight tiles in registers, the batch is the N dimension of the MFMA).  None: on (env T2V_PERSIST16=0 switches it
    # off); False: off; 'force': also for B <= 6, where the fp32-weight kernel is the default (tests)
    persistent16 = None
    # ---- what the most recent call ran on (written by _note() alone; bench / tests / tools read them)
    keep_last = False       # bench / tests: keep the (first chunk's) arena of the last forward for replays
    last_call = None        # keep_last: (weights, bufs, dims, arena + constants) of the first chunk of the last forward
    last_persist = None     # keep_last: (weights, bufs, scratch, dims, tensors) of the last persistent forward, for replays
    last_bwd = None         # keep_last: the same for the launch-per-step / ...
    last_bwd_persist = None     # ... the one-launch reverse pass of the first chunk
    last_persist_engine = last_bwd_persist_engine = None    # key of the engine the chunk of last_persist / last_bwd_persist ran on
    dw_tile_cap = None      # tests: at most this many tiles in the weight-gradient epilogue of a reverse pass (None: no cap)
    last_mode = None        # 'persistent' | 'launch-per-step' of the most recent forward chunk
    last_bwd_mode = None
    last_kernel = None      # name of the forward kernel of the most recent chunk
    last_bwd_kernel = None
    chunk_kernels = []      # forward kernel of every chunk of the most recent forward, in batch order (a step can mix them)
    chunk_bwd_kernels = []  # ... and of the most recent reverse pass

    @staticmethod
    def plan(lib, B, T_in, T, need_grad):
        """The kernels of one call: a ChunkPlan per chunk of <= MAX_DEC_B items.  The only reader of the class switches, of
        bf16_run and of T2V_TRAIN_PERSISTENT / T2V_BWD_PERSISTENT / T2V_PERSIST16 / T2V_PERSIST16_BWD, and the only caller of
        the library's *_supported / *_fits / *_scratch_floats queries.  A class switch that is not None wins over its variable.

        Switches.  Forward: DecoderCore.persistent, else T2V_TRAIN_PERSISTENT != '0'.  Reverse: DecoderCore.persistent_bwd, else
        T2V_BWD_PERSISTENT != '0', which defaults to T2V_TRAIN_PERSISTENT (measured, B = 6, T_in = 84, T = 400, round 3: 12.9 us
        per reverse step against 18.2 for the launch-per-step pass; both kernels want the GPU to themselves).  bf16 kernels:
        DecoderCore.persistent16, else T2V_PERSIST16 != '0'; they exist under bf16_run only.

        Forward engine of a chunk of b items:
          'persist'    forward switch on, t2v_decoder_train_persist_supported(b, T_in) (b <= 6, T_in <= 560), and its scratch
                       below 2^31 - 1 bytes (31-bit buffer offsets);
          'persist16'  bf16 switch and forward switch on, t2v_decoder_train_persist16_supported(b, T_in) (b <= 16), scratch
                       below 2^31 - 1 bytes — and 'persist' not possible, unless persistent16 == 'force';
          'steps'      otherwise (launch per step).
        Reverse engine of a chunk (need_grad only; None without):
          'achain'     reverse switch on, t2v_decoder_bwd_persist_supported(b, T_in) (b <= 6, T_in <= 576), scratch below
                       2^31 - 1 bytes;
          'persist16'  bf16 switch on, T2V_PERSIST16_BWD != '0', reverse switch on, t2v_decoder_bwd_persist16_fits(b, T_in, T)
                       (supported AND every exchange array below the kernel's 31-bit buffer offsets at this T: a long
                       utterance leaves it HERE, not after the forward) — and 'achain' not possible, unless 'force';
          'steps'      otherwise — and then for EVERY chunk of the call: the launch-per-step pass reads transposed weight
                       packs that one call either builds or does not.
        The 16 forward follows the forward switch, the 16 reverse pass the reverse switch.  The preparation of a one-launch
        reverse pass is issued behind the forward launch when that chunk's forward is a persistent kernel too.
        Weight-gradient epilogue (dw_epilogue): 'achain' chunks of an fp32 run whose LSTM weight gradients take the grouped
        plane launch — not under bf16_run, T2V_F32_GEMM=native or T2V_DW_GROUPED=0; T2V_DW_EPILOGUE=0 switches it off."""
        D = DecoderCore
        env = os.environ.get
        fwd_on = D.persistent if D.persistent is not None else env('T2V_TRAIN_PERSISTENT', '1') != '0'
        bwd_on = D.persistent_bwd if D.persistent_bwd is not None else env('T2V_BWD_PERSISTENT', env('T2V_TRAIN_PERSISTENT', '1')) != '0'
        on16 = D.persistent16 if D.persistent16 is not None else env('T2V_PERSIST16', '1') != '0'
        force = on16 == 'force'
        on16 = bool(on16) and bool(_BF16)
        small = lambda floats: 4 * floats < 2 ** 31 - 1
        chunks = [(b0, min(B, b0 + MAX_DEC_B)) for b0 in range(0, B, MAX_DEC_B)]
        fwd, bwd = [], []
        for b0, b1 in chunks:
            b = b1 - b0
            p32 = bool(fwd_on) and bool(lib.t2v_decoder_train_persist_supported(b, T_in)) and \
                small(lib.t2v_decoder_train_persist_scratch_floats(b, T_in, T))
            f16 = on16 and bool(fwd_on) and bool(lib.t2v_decoder_train_persist16_supported(b, T_in)) and (force or not p32) and \
                small(lib.t2v_decoder_train_persist16_scratch_floats(b, T_in, T))
            fwd.append('persist16' if f16 else 'persist' if p32 else 'steps')
            if need_grad:
                r32 = bool(bwd_on) and bool(lib.t2v_decoder_bwd_persist_supported(b, T_in)) and \
                    small(lib.t2v_decoder_bwd_achain_scratch_floats(b, T_in, T))
                r16 = on16 and env('T2V_PERSIST16_BWD', '1') != '0' and bool(bwd_on) and \
                    bool(lib.t2v_decoder_bwd_persist16_fits(b, T_in, T)) and (force or not r32)
                bwd.append('persist16' if r16 else 'achain' if r32 else 'steps')
            else:
                bwd.append(None)
        if 'steps' in bwd:
            bwd = ['steps'] * len(bwd)
        dw_on = (not _BF16 and env('T2V_DW_EPILOGUE', '1') != '0' and env('T2V_DW_GROUPED', '1') != '0' and
                 env('T2V_F32_GEMM', '') not in ('native', '0'))
        return [ChunkPlan(b0, b1, f, r, f != 'steps' and r in _BWD_ENGINES, dw_on and r == 'achain')
                for (b0, b1), f, r in zip(chunks, fwd, bwd)]

    @staticmethod
    def _note(fwd=None, bwd=None, **kept):
        """The one place that records what ran: the engine of a forward / reverse chunk, and the keep_last records by name."""
        D = DecoderCore
        if fwd is not None:
            D.last_mode = 'launch-per-step' if fwd == 'steps' else 'persistent'
            D.last_kernel = _STEPS_KERNELS['fwd'] if fwd == 'steps' else _FWD_ENGINES[fwd].kernel
            D.chunk_kernels.append(D.last_kernel)
        if bwd is not None:
            D.last_bwd_mode = 'launch-per-step' if bwd == 'steps' else 'persistent'
            D.last_bwd_kernel = _STEPS_KERNELS['bwd'] if bwd == 'steps' else _BWD_ENGINES[bwd].kernel
            D.chunk_bwd_kernels.append(D.last_bwd_kernel)
        for name, value in kept.items():
            setattr(D, name, value)

    @staticmethod
    def _wgrad_tensors(ctx, f32):
        """gradient tensors of the four nn.LSTMCell weights (arena slots when FlatAdam registered them)"""
        if ctx.wg is None:       # made where a backward first needs them: in front of a pass with an epilogue, else in _chunk_grads
            wg = [grad_slot(w) for w in ctx.wrefs]
            ctx.wg = [torch.empty(w.shape, **f32) if g is None else g for g, w in zip(wg, ctx.wrefs)]
        return ctx.wg

    @staticmethod
    def _dw_groups(DGA, DGD, XS, wg, pre_c, T, B):
        """the five LSTM weight-gradient products of a chunk as the two groups of gemm_grouped"""
        TB = T * B
        x_prev, x_cur = XS[0:T].reshape(TB, XW), XS[1:T + 1].reshape(TB, XW)
        d_w_ih_att, d_w_hh_att, d_w_ih_dec, d_w_hh_dec = wg
        att = [(x_prev[:, :H].t(), d_w_hh_att), (x_prev[:, H:KATT].t(), d_w_ih_att[:, PRE:])]
        if pre_c is not None:
            att.insert(0, (pre_c.t(), d_w_ih_att[:, :PRE]))
        return [(DGA.view(TB, G4).t(), att), (DGD.view(TB, G4).t(), [(x_cur[:, :KATT].t(), d_w_ih_dec), (x_cur[:, KATT:].t(), d_w_hh_dec)])]

    @staticmethod
    def _bwd_buffers(lib, eng, B, T_in, T, dev):
        """dq partials, scratch and error word of a one-launch reverse pass"""
        f32 = dict(device=dev, dtype=torch.float32)
        DQP = torch.empty(T, B, getattr(lib, eng.slices)(T_in), A, **f32)
        scratch = torch.empty(getattr(lib, eng.scratch)(B, T_in, T), **f32)
        return DQP, scratch, torch.zeros(1, device=dev, dtype=torch.int32)

    @staticmethod
    def _fwd_chunk(lib, plan, gpre, memory, pm, lengths, packs, bias_dec, wqT, wcomb, vv, need_grad, p_att, p_dec, seed, wbf, raw):
        T, B, _ = gpre.shape
        T_in = memory.shape[1]
        f32 = dict(device=gpre.device, dtype=torch.float32)
        # row 0 of the state arenas (zero initial states) is cleared by the library's one reset launch
        XS = torch.empty(T + 2, B, XW, **f32)
        CA = torch.empty(T + 1, B, H, **f32)
        CD = torch.empty(T + 1, B, H, **f32)
        GA = torch.empty(T, B, G4, **f32) if need_grad else None
        GD = torch.empty(T, B, G4, **f32) if need_grad else None
        QP = torch.empty(lib.t2v_decoder_qp_floats(B, T_in), **f32)
        AL = torch.empty(T + 1, B, T_in, **f32)
        ACUM = torch.empty(T + 1, B, T_in, **f32)
        S = torch.empty(T, B, T_in, A, **f32) if need_grad else None
        keep = (gpre, memory, pm, lengths, XS, CA, CD, GA, GD, QP, AL, ACUM, S)          # the order of _ARENA
        packF_att, packF_dec, packB_att, packB_dec = packs
        W = _DecWeights(_p(packF_att), _p(packF_dec), _p(packB_att), _p(packB_dec), None, _p(bias_dec),
                        _p(wqT), _p(wcomb), _p(vv), int(bool(wbf)))
        Sb = _DecTrainBufs(*(_p(t) for t in keep))
        dims = (B, T_in, T, float(p_att), float(p_dec), int(seed))
        if plan.fwd == 'steps':
            _check(lib.t2v_decoder_train_fwd(C.byref(W), C.byref(Sb), *(dims + (_stream(),))), 't2v_decoder_train_fwd')
            _err_note('decoder forward (attention exchange)', QP.view(torch.int32)[B * 256 * A + 31:][:1])
            DecoderCore._note(fwd='steps')
            return W, Sb, keep, None
        eng = _FWD_ENGINES[plan.fwd]
        scratch = torch.empty(getattr(lib, eng.scratch)(B, T_in, T), **f32)
        PW = _persist_weights(raw, bias_dec, wcomb, vv)
        _check(getattr(lib, eng.run)(C.byref(PW), C.byref(Sb), _p(scratch), *(dims + (_stream(),))), eng.run)
        _err_note('decoder forward (persistent kernel hand-off)', QP.view(torch.int32)[B * 256 * A + 31:][:1])
        DecoderCore._note(fwd=plan.fwd)
        if DecoderCore.keep_last:
            DecoderCore._note(last_persist=(PW, Sb, scratch, dims, raw), last_persist_engine=plan.fwd)
        if not plan.prepare:
            return W, Sb, keep, None
        # the preparation of the reverse pass (sentinel fills — 1.4 MB per time step for the bf16 pass — and, for the fp32 pass,
        # the factor arrays of both cells: ~150 us of launches that need nothing but this forward pass) goes out NOW, on the
        # deferred-work stream, next to the Postnet.  (round 5, measured: issued at the TOP of the step instead, next to the
        # encoder, the step time does not change — 12.90 vs 12.91 ms — so the buffers are not held for the whole forward pass)
        beng = _BWD_ENGINES[plan.bwd]
        DQP, bscr, errw = DecoderCore._bwd_buffers(lib, beng, B, T_in, T, gpre.device)
        with side('w', keep=tuple(keep[_ARENA.index(n)] for n in beng.keep)):
            args = (_p(DQP), _p(bscr), _p(errw), B, T_in, T)
            if beng.arena_prepare:
                args = (C.byref(Sb),) + args + dims[3:]
            _check(getattr(lib, beng.prepare)(*(args + (_stream(),))), beng.prepare)
            ev = torch.cuda.Event()
            ev.record()
        # (the prepared buffers travel with the chunk on the autograd ctx — a process-wide table keyed by id(XS) could hand
        # a later chunk the scratch of a forward pass whose backward never ran)
        return W, Sb, keep, (DQP, bscr, errw, ev)

    @staticmethod
    def forward(ctx, gpre, memory, pm, lengths, w_ih_att, w_hh_att, w_ih_dec, w_hh_dec, bias_dec,
                wq, loc_conv, loc_dense, v, p_att, p_dec, seed, grad_mode=True, pre=None, b_ih_att=None, b_hh_att=None,
                gpre_ready=None):
        lib = _require_gpu(memory, pm, w_ih_att)
        pre2 = None
        if pre is not None:
            # gpre = pre · weight_ih[:, :256]^T + b_ih + b_hh computed here (gpre argument None), so attention_rnn.weight_ih
            # has ONE gradient producer and its prenet columns are written in place by the backward
            assert gpre is None
            pre2 = _f32c(pre).view(-1, PRE)
            if gpre_ready is not None:      # the same product, issued earlier on a side stream (Decoder.prepare)
                gpre = gpre_ready.view(pre.shape[0], pre.shape[1], G4)
            else:
                gpre = gemm(pre2, w_ih_att.detach()[:, :PRE], (b_ih_att + b_hh_att).detach()).view(pre.shape[0], pre.shape[1], G4)
        T, B, _ = gpre.shape
        T_in = memory.shape[1]
        gpre, memory, pm = _f32c(gpre), _f32c(memory), _f32c(pm)
        # grad_mode = torch.is_grad_enabled() of the CALLER (inside Function.forward it is always False): under
        # no_grad (validate(), inference) nothing is saved and the backward-only buffers are not even allocated
        need_grad = bool(grad_mode) and any(ctx.needs_input_grad)
        wbf = bool(_BF16)
        plans = DecoderCore.plan(lib, B, T_in, T, need_grad)
        # the persistent kernels read the nn.LSTMCell tensors themselves; the forward packs are only built when some chunk
        # takes the launch-per-step forward, the transposed packs when the reverse pass is the launch-per-step one
        fwd_persist = all(p.fwd != 'steps' for p in plans)
        bwd_persist = need_grad and all(p.bwd != 'steps' for p in plans)
        if fwd_persist and (bwd_persist or not need_grad):
            packs = (None, None, None, None)
        else:
            packs = pack_decoder_weights(w_ih_att, w_hh_att, w_ih_dec, w_hh_dec, KATT, need_grad and not bwd_persist, bf16=wbf,
                                         need_fwd=not fwd_persist)
        raw = tuple(_f32c(t.detach()) for t in (w_ih_att, w_hh_att, w_ih_dec, w_hh_dec, wq))
        wqT = wq.detach().t().contiguous()
        bias_dec = _f32c(bias_dec.detach())
        loc_conv, loc_dense, vv = _f32c(loc_conv.detach()), _f32c(loc_dense.detach()), _f32c(v.detach()).view(-1)
        wcomb = fuse_location_weights(loc_conv, loc_dense)
        chunks = []
        DecoderCore._note(chunk_kernels=[])
        for p in plans:
            if p.b0 == 0 and p.b1 == B:
                g_c, m_c, pm_c, l_c = gpre, memory, pm, lengths
            else:
                g_c, m_c, pm_c = gpre[:, p.b0:p.b1].contiguous(), memory[p.b0:p.b1].contiguous(), pm[p.b0:p.b1].contiguous()
                l_c = None if lengths is None else lengths[p.b0:p.b1].contiguous()
            chunks.append(DecoderCore._fwd_chunk(lib, p, g_c, m_c, pm_c, l_c, packs, bias_dec, wqT, wcomb, vv, need_grad,
                                                 p_att, p_dec, _chunk_seed(seed, p.b0), wbf, raw))
        hcs = []
        for _w, _s, k, _prep in chunks:          # (h_dec(t), context(t)) rows of the projection, gathered from the arena in one launch
            XSc = k[4]
            Bc, XWc = XSc.size(1), XSc.size(2)
            hc_c = torch.empty(T, Bc, XWc - H, device=XSc.device, dtype=torch.float32)
            _check(lib.t2v_concat2_rows(_p(XSc[2:, :, KATT:]), XWc, XWc - KATT, _p(XSc[1:, :, H:KATT]), XWc, KATT - H, _p(hc_c),
                                        T * Bc, _stream()), 't2v_concat2_rows')
            hcs.append(hc_c)
        als = [k[10][1:].permute(1, 0, 2) for _, _, k, _ in chunks]
        HC, align = _cat(hcs, 1), _cat(als, 0)
        ctx.dims = (B, T_in, T, float(p_att), float(p_dec), int(seed))
        ctx.consts = (packs, bias_dec, wqT, wcomb, vv, loc_conv, loc_dense)
        ctx.wbf = wbf
        ctx.wrefs = (w_ih_att, w_hh_att, w_ih_dec, w_hh_dec)
        ctx.raw = raw
        ctx.pre2 = pre2
        ctx.pre_on_side = gpre_ready is not None     # Decoder.prepare ran the Prenet on the engine's deferred-work stream
        ctx.plans = plans
        ctx.chunks = [k for _, _, k, _ in chunks] if need_grad else None
        ctx.prepared = [pr for _, _, _, pr in chunks] if need_grad else None
        ctx.set_materialize_grads(False)        # an output without a gradient arrives in backward as None, not as zeros
        if DecoderCore.keep_last:
            W0, S0, k0, _ = chunks[0]
            DecoderCore._note(last_call=(W0, S0, (k0[0].shape[1], T_in, T, float(p_att), float(p_dec), int(seed)),
                                         k0 + (packs, bias_dec, wqT, wcomb, vv)))
        return HC, align

    @staticmethod
    def _pre_chunk(ctx, b0, B):
        """the chunk's rows of the Prenet output as (T * B, 256); None when the Prenet is not folded into this node"""
        Bt, _, T = ctx.dims[:3]
        return ctx.pre2 if ctx.pre2 is None or B == Bt else ctx.pre2.view(T, Bt, PRE)[:, b0:b0 + B].reshape(T * B, PRE)

    @staticmethod
    def _bwd_persist(ctx, lib, ci, dhc_c, dal_c, DGA, DGD, DCTX):
        """The reverse pass of chunk ci as ONE persistent launch (csrc/decoder_train_bwd_persist.hip; bf16_run, B <= 16: on bf16
        MFMA tiles, csrc/decoder_train_bwd_persist16.hip).  Returns DV, dq_sum (T * B, 128) and the GroupedHandOver of the
        chunk's weight-gradient epilogue (None: the pass has none)."""
        plan, keep, b0, B = ctx.plans[ci], ctx.chunks[ci], ctx.plans[ci].b0, DGA.size(1)
        _, T_in, T, p_att, p_dec, seed = ctx.dims
        _packs, bias_dec, _wqT, wcomb, vv = ctx.consts[:5]
        eng = _BWD_ENGINES[plan.bwd]
        f32 = dict(device=dhc_c.device, dtype=torch.float32)
        # (a one-launch reverse pass has its own slice geometry, e.g. one workgroup per item up to 96 symbols)
        DV = torch.empty(B, getattr(lib, eng.slices)(T_in), A, **f32)
        Sb = _DecTrainBufs(*(_p(t) for t in keep))
        PW = _persist_weights(ctx.raw, bias_dec, wcomb, vv)
        prep, ctx.prepared[ci] = ctx.prepared[ci], None
        if prep is not None:
            DQP, scratch, errw, pev = prep
            torch.cuda.current_stream().wait_event(pev)     # (always: the preparation ran on a side stream)
        else:
            DQP, scratch, errw = DecoderCore._bwd_buffers(lib, eng, B, T_in, T, dhc_c.device)
        dwh = None
        if plan.dw_epilogue and set_f32_gemm_mode(None) and T * B >= 32:
            # the decoder_rnn workgroups go on with decoder_rnn's weight gradients when their chain has ended: the gradient
            # tensors, the grouped launch's scratch and its groups have to exist before the pass
            groups = DecoderCore._dw_groups(DGA, DGD, keep[4], DecoderCore._wgrad_tensors(ctx, f32), DecoderCore._pre_chunk(ctx, b0, B), T, B)
            dwh = GroupedHandOver(groups, 1, scratch[lib.t2v_decoder_bwd_achain_dw_offset(B, T_in, T):][:1], ci > 0, DecoderCore.dw_tile_cap)
            if ci > 0 and overlap() is not None:
                # this pass adds to d_w_*_dec on the current stream; the tiles an earlier chunk left over were added by its
                # grouped launch on the deferred-GEMM stream
                overlap().wait('g')
        stamp('dec_bwd_begin')
        bufs = (dhc_c, DGA, DGD, DCTX, DV, DQP, scratch, errw)
        _bwd_launch(lib, eng, prep is not None, PW, Sb, bufs, (B, T_in, T, p_att, p_dec, _chunk_seed(seed, b0)),
                    None if dwh is None else dwh.dw, dal_c)
        _err_note('decoder backward (persistent kernel hand-off)', errw)
        dq_off = getattr(lib, eng.dq_offset)(B, T_in, T)       # slice 0 of every item has summed the slices already
        rows = eng.dq_rows or B
        dq_sum = scratch[dq_off:dq_off + T * rows * A].view(T, rows, A)[:, :B].reshape(T * B, A)
        DecoderCore._note(bwd=plan.bwd)
        if DecoderCore.keep_last and b0 == 0:
            DecoderCore._note(last_bwd_persist=(PW, Sb, bufs, (B, T_in, T, p_att, p_dec, seed), keep + (ctx.raw, wcomb, vv, bias_dec, dwh)),
                              last_bwd_persist_engine=plan.bwd)
        return DV, dq_sum, dwh

    @staticmethod
    def _bwd_step_buffers(lib, B, T_in, T, NS, dev):
        """dq partials, the cells' carried state and the attention hand-off words of a launch-per-step reverse pass"""
        f32 = dict(device=dev, dtype=torch.float32)
        tcap = (T_in + 15) // 16 * 16
        DQ = torch.empty(T, B, NS, A, 2, **f32)
        YD, YA, DCA, DCD = (torch.empty(B, n, **f32) for n in (XW, KATT, H, H))
        GPREV, GCUM = torch.empty(2, B, NS, 2, 64, **f32), torch.empty(B * NS * tcap + 64, **f32)
        return DQ, YD, YA, DCA, DCD, GPREV, GCUM, GCUM.view(torch.int32)[B * NS * tcap + 1:][:1]

    @staticmethod
    def _bwd_steps(ctx, lib, ci, dhc_c, dal_c, DGA, DGD, DCTX):
        """The reverse pass of chunk ci as one launch pair per step (k_lstm_bwd256 + k_attn_cell_bwd).  Returns DV, dq_sum
        (T * B, 128) and None (no weight-gradient epilogue)."""
        keep, b0, B = ctx.chunks[ci], ctx.plans[ci].b0, DGA.size(1)
        _, T_in, T, p_att, p_dec, seed = ctx.dims
        packs, bias_dec, wqT, wcomb, vv = ctx.consts[:5]
        NS = lib.t2v_attn_bwd_slices(T_in)
        DV = torch.empty(B, NS, A, device=dhc_c.device, dtype=torch.float32)
        Sb = _DecTrainBufs(*(_p(t) for t in keep))
        W = _DecWeights(*(_p(t) for t in packs), None, _p(bias_dec), _p(wqT), _p(wcomb), _p(vv), int(bool(ctx.wbf)))
        DQ, YD, YA, DCA, DCD, GPREV, GCUM, errw = DecoderCore._bwd_step_buffers(lib, B, T_in, T, NS, dhc_c.device)
        gb = (dhc_c, DGA, DGD, DQ, DCTX, YD, YA, DCA, DCD, GPREV, GCUM, DV)             # the fields of t2v_dec_bwd_bufs
        Gb = _DecBwdBufs(*(_p(t) for t in gb))
        if dal_c is None:
            _check(lib.t2v_decoder_train_bwd(C.byref(W), C.byref(Sb), C.byref(Gb), B, T_in, T, p_att, p_dec,
                                             _chunk_seed(seed, b0), _stream()), 't2v_decoder_train_bwd')
        else:
            _check(lib.t2v_decoder_train_bwd_align(C.byref(W), C.byref(Sb), C.byref(Gb), _p(dal_c), B, T_in, T, p_att, p_dec,
                                                   _chunk_seed(seed, b0), _stream()), 't2v_decoder_train_bwd_align')
        _err_note('decoder backward (dq hand-off)', errw)
        dq_sum = DQ[..., 0].sum(2).view(T * B, A)
        DecoderCore._note(bwd='steps')
        if DecoderCore.keep_last and b0 == 0:
            DecoderCore._note(last_bwd=(W, Sb, Gb, (B, T_in, T, p_att, p_dec, seed),
                                        keep + gb + (packs, bias_dec, wqT, wcomb, vv)))
        return DV, dq_sum, None

    @staticmethod
    def _chunk_grads(ctx, lib, ci, dhc_c, DGA, DGD, DCTX, DV, dq_sum, dwh, acc, dpre_l):
        """The gradients of chunk ci, behind its reverse pass.  Returns d_memory, d_pm, acc + the chunk's [d_wq, d_loc_conv, d_loc_dense,
        d_v] (acc: the earlier chunks' sums, None for chunk 0; added on the deferred-work stream, where they are made) and the bias
        gradients.  The LSTM weight gradients go into _wgrad_tensors (chunk 0 writes, later ones add), a Prenet data gradient to dpre_l."""
        keep, b0, B, first = ctx.chunks[ci], ctx.plans[ci].b0, DGA.size(1), ci == 0
        XS, AL, ACUM, dpre = keep[4], keep[10], keep[11], keep[12]      # S: overwritten in place by the backward kernels
        (T_in, T), (loc_conv, loc_dense) = ctx.dims[1:3], ctx.consts[5:]
        TB = T * B
        f32 = dict(device=dhc_c.device, dtype=torch.float32)
        dga2 = DGA.view(TB, G4)
        stamp('dec_bwd_end')
        fork = mark()
        # ---- what the encoder's backward waits for stays on the current stream ...
        d_memory = torch.empty(B, T_in, E, **f32)
        # per item: alpha_b^T (T_in x T) · dctx_b (T x 512), all items in one launch
        _check(lib.t2v_gemm_f32_batched(_p(AL[1:]), T_in, 1, B * T_in, _p(DCTX), E, 1, B * E, _p(d_memory), T_in * E, E, B,
                                        T_in, E, T, _stream()), 't2v_gemm_f32_batched')
        d_pm = colsum(dpre.view(T, B * T_in * A)).view(B, T_in, A)
        want_dpre = ctx.pre2 is not None and ctx.needs_input_grad[17]
        if want_dpre and not ctx.pre_on_side:
            # the Prenet ran on the caller's stream: its backward is ordered behind THIS stream only
            dpre_l.append(gemm(dga2, ctx.wrefs[0].detach()[:, :PRE].t()).view(T, B, PRE))
        # ---- ... every weight gradient goes to the engine's deferred-work stream (inline without an engine): the
        # ≈ 80 GFLOP of time-batched LSTM weight-gradient GEMMs then run next to the BiLSTM / reference-encoder
        # backward chains instead of in front of them
        with side('w', keep=(DGA, DGD, DCTX, DV, dq_sum, dhc_c) + tuple(keep), after=fork):
            wg = DecoderCore._wgrad_tensors(ctx, f32)
            if first and ctx.pre2 is None:      # the prenet columns of attention_rnn.weight_ih get their gradient via gpre
                wg[0][:, :PRE].zero_()
            # round 6: the five LSTM weight-gradient products as ONE launch of the plane kernel — both gate-gradient operands split
            # (fp32: x3 planes; bf16_run: rounded) once, 1 024 tiles = two full rounds of the chip (T2V_DW_GROUPED=0: one by one)
            grouped = os.environ.get('T2V_DW_GROUPED', '1') != '0'
            groups = dwh.groups if dwh is not None else DecoderCore._dw_groups(DGA, DGD, XS, wg, DecoderCore._pre_chunk(ctx, b0, B), T, B)
            products = [(gt, xt, out) for gt, parts in groups for xt, out in parts]        # _dw_groups' order
            if ctx.pre2 is not None:    # the input projection of the prenet output, folded into this node: the Prenet's
                # own backward (issued on this same stream when an engine is active) waits for d_pre, so it goes first
                if want_dpre and ctx.pre_on_side:
                    dpre_l.append(gemm(dga2, ctx.wrefs[0].detach()[:, :PRE].t()).view(T, B, PRE))
                if not grouped:         # (one by one: the Prenet columns' product stays on this stream)
                    gt, xt, out = products.pop(0)
                    gemm(gt, xt, out=out, accumulate=not first)
            # each product lands in its own tensor (no split / copy afterwards).  fp32: the own large-tile fp32 MFMA GEMM;
            # bf16_run: the own large-tile bf16 GEMM (k_gemm_bf16_big_rr: operands rounded to bf16 while staged, fp32
            # accumulation) — no library GEMM is left in either step.  (What they cost on the step's clock: DESIGN §4.1)
            with side('g', after=fork, keep=() if dwh is None else (dwh.scr,)):
                if dwh is not None:
                    # (the pass has written the decoder_rnn group's planes and taken tiles of it: this launch does the rest)
                    gemm_grouped(groups, accumulate=not first, handed=dwh)
                elif grouped:
                    gemm_grouped(groups, accumulate=not first)
                else:
                    for gt, xt, out in products:
                        gemm(gt, xt, out=out, accumulate=not first)
            # the attention weight gradients stay on the deferred-work stream: on a stream of their own they are a fifth concurrent
            # branch on the graph executor's four queues, which costs more than the shorter path buys (measured)
            d_wq = gemm(dq_sum.t(), XS[1:T + 1].reshape(TB, XW)[:, :H].t())            # (128,1024), from h_att_t
            d_v = DV.sum((0, 1)).view(1, A)
            d_loc_dense, d_loc_conv = attn_wgrad(dpre, AL, ACUM, loc_conv, loc_dense, B, T_in, T)
            parts = [d_wq, d_loc_conv, d_loc_dense, d_v]
            acc = parts if acc is None else [x + y for x, y in zip(acc, parts)]
        # bias gradients flow on through an Add node (bias_ih + bias_hh) / are handed to two inputs: node's stream
        return d_memory, d_pm, acc, [colsum(DGD.view(TB, G4))] + ([colsum(dga2)] if ctx.pre2 is not None else [])

    @staticmethod
    def _dal_chunk(dalign, b0, B, Bt):
        """rows [b0, b0 + B) of the alignment gradient (Bt, T, T_in) as the kernels read them: contiguous (T, B, T_in).  No copy
        when the call has one chunk and the tensor is a (B, T, T_in) view of such storage (what guided_attention writes)."""
        if dalign is None:
            return None
        tb = dalign.permute(1, 0, 2)
        if B == Bt and tb.is_contiguous():
            return tb
        return tb[:, b0:b0 + B].contiguous()

    @staticmethod
    def backward(ctx, dHC, dalign):
        """The chunk loop: each chunk's reverse pass (_bwd_persist | _bwd_steps, as plan() chose), its gradients
        (_chunk_grads), the sums over the chunks and the return tuple.  dHC / dalign: None for an output the loss did not use."""
        lib = load_library()
        if ctx.chunks is None:
            raise T2VHipError("DecoderCore.backward without a saved arena (forward ran under no_grad)")
        Bt, T_in, T = ctx.dims[:3]
        dev = ctx.chunks[0][4].device
        f32 = dict(device=dev, dtype=torch.float32)
        dHC = torch.zeros(T, Bt, H + E, **f32) if dHC is None else _f32c(dHC)
        if dalign is not None:
            assert dalign.dtype == torch.float32 and dalign.shape == (Bt, T, T_in), (dalign.dtype, tuple(dalign.shape))
        acc = bacc = ctx.wg = None
        dga_l, dmem_l, dpm_l, dpre_l = [], [], [], []
        DecoderCore._note(chunk_bwd_kernels=[])
        for ci, plan in enumerate(ctx.plans):
            b0, B = plan.b0, plan.b1 - plan.b0
            dhc_c = dHC if B == Bt else dHC[:, b0:b0 + B].contiguous()
            DGA, DGD, DCTX = torch.empty(T, B, G4, **f32), torch.empty(T, B, G4, **f32), torch.empty(T, B, E, **f32)
            reverse = DecoderCore._bwd_persist if plan.bwd in _BWD_ENGINES else DecoderCore._bwd_steps
            dal_c = DecoderCore._dal_chunk(dalign, b0, B, Bt)
            rev = reverse(ctx, lib, ci, dhc_c, dal_c, DGA, DGD, DCTX)       # DV, dq_sum, the epilogue's hand-over
            d_memory, d_pm, acc, bparts = DecoderCore._chunk_grads(ctx, lib, ci, dhc_c, DGA, DGD, DCTX, *rev, acc, dpre_l)
            bacc = bparts if bacc is None else [x + y for x, y in zip(bacc, bparts)]
            dmem_l.append(d_memory); dpm_l.append(d_pm); dga_l.append(DGA)
        ctx.chunks = ctx.prepared = None   # the arena is released as soon as the backward has consumed it (side-stream readers: keep=)
        wg, ctx.wg = ctx.wg, None          # d_w_ih_att, d_w_hh_att, d_w_ih_dec, d_w_hh_dec; acc: d_wq, d_loc_conv, d_loc_dense, d_v
        d_memory, d_pm = _cat(dmem_l, 0), _cat(dpm_l, 0)
        DGA = d_pre = d_b_att = None
        if ctx.pre2 is not None:
            d_b_att = bacc[1]
            if dpre_l and ctx.pre_on_side:
                with side('w'):
                    d_pre = _cat(dpre_l, 1)
            elif dpre_l:
                d_pre = _cat(dpre_l, 1)
        else:
            DGA = _cat(dga_l, 1)
        return (DGA, d_memory, d_pm, None, *wg, bacc[0], *acc, None, None, None, None, d_pre, d_b_att, d_b_att, None)


def attn_wgrad(dpre, AL, ACUM, loc_conv, loc_dense, B, T_in, T):
    """location_dense / location_conv weight gradients summed over the whole decoder pass (csrc/attn_wgrad.hip)."""
    lib = _require_gpu(dpre, AL, ACUM, loc_conv, loc_dense)
    f32 = dict(device=dpre.device, dtype=torch.float32)
    part = torch.empty(lib.t2v_attn_wgrad_scratch_floats(), **f32)
    d_dense, d_conv = torch.empty(A, F_LOC, **f32), torch.empty(F_LOC, 2, KS, **f32)
    _check(lib.t2v_attn_wgrad(_p(dpre), _p(AL), _p(ACUM), _p(_f32c(loc_conv)), _p(_f32c(loc_dense)), _p(part),
                              _p(d_dense), _p(d_conv), B, T_in, T, _stream()), 't2v_attn_wgrad')
    return d_dense, d_conv


def mel_frontend(wav, n_samples, tables, scale=1.0, t_stride=None):
    """Batched STFT→mel on device.  wav: (B,N) float32 or int16 CUDA tensor; n_samples: (B) int64.
    tables: dict from layers.TacotronSTFT (device tensors).  Returns (B,80,T_max) float32."""
    lib = _require_gpu(wav)
    B, N = wav.shape
    wav = wav.contiguous()
    if int(n_samples.min()) <= 512 or int(n_samples.max()) > N:
        # reflect padding of n_fft/2 needs more than n_fft/2 samples (torch raises for the reference's F.pad too)
        raise ValueError("mel_frontend: every utterance needs 512 < n_samples <= %d, got [%d, %d]"
                         % (N, int(n_samples.min()), int(n_samples.max())))
    n_samples = n_samples.to(device=wav.device, dtype=torch.int64).contiguous()
    if t_stride is None:
        t_stride = int(n_samples.max().item()) // 256 + 1
    out = torch.empty(B, 80, t_stride, device=wav.device, dtype=torch.float32)
    is16 = wav.dtype == torch.int16
    if not is16 and wav.dtype != torch.float32:
        raise T2VHipError("mel_frontend takes float32 or int16 samples")
    _check(lib.t2v_mel_frontend(None if is16 else _p(wav), _p(wav) if is16 else None, _p(n_samples), B, N,
                                float(scale), 1024, 256, 80, _p(tables['window']), _p(tables['tw512']),
                                _p(tables['tw1024']), _p(tables['mel_start']), _p(tables['mel_len']),
                                _p(tables['mel_w']), int(tables['maxw']), _p(out), t_stride, _stream()),
           't2v_mel_frontend')
    return out


class CorpusStore(object):
    """The device side of corpus.ResidentCorpus, as t2v_collate_batch reads it (include/t2vae.h): flat fp32 mels with int64
    offsets, flat int32 symbol ids with int64 offsets, and one int32 per utterance for the frame count, the symbol count, the
    speaker and the emotion.  host_frames / host_ids are the same counts on the host (CPU int64 tensors): every check of a
    batch runs on them, never on device memory."""
    TENSORS = ('mel', 'mel_off', 'n_frames', 'ids', 'id_off', 'n_ids', 'speaker', 'emotion')
    DTYPES = (torch.float32, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int32)

    def __init__(self, n_speakers, n_emotions, host_frames, host_ids, **tensors):
        self.n_speakers, self.n_emotions = int(n_speakers), int(n_emotions)
        self.host_frames, self.host_ids = host_frames, host_ids
        self.n_utts = int(host_frames.numel())
        for name, dt in zip(self.TENSORS, self.DTYPES):
            t = tensors[name]
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise T2VHipError("CorpusStore.%s: a contiguous %s device tensor is needed" % (name, dt))
            setattr(self, name, t)
        for name in self.TENSORS:
            if name not in ('mel', 'ids') and getattr(self, name).numel() != self.n_utts:
                raise T2VHipError("CorpusStore.%s: %d entries for %d utterances" % (name, getattr(self, name).numel(), self.n_utts))

    def nbytes(self):
        return sum(getattr(self, n).numel() * getattr(self, n).element_size() for n in self.TENSORS)


def collate_check(store, indices, T_in, T_out):
    """the host's check of one batch against the store's host tables: ValueError, nothing launched.  Returns the indices as a list."""
    indices = [int(i) for i in (indices.tolist() if torch.is_tensor(indices) else indices)]
    if not indices:
        raise ValueError("collate_batch: an empty batch")
    if min(indices) < 0 or max(indices) >= store.n_utts:
        raise ValueError("collate_batch: utterance indices must lie in [0, %d), got %s" % (store.n_utts, indices))
    need_in = int(store.host_ids[indices].max())
    need_out = int(store.host_frames[indices].max())
    if T_in < need_in or T_out < need_out:
        raise ValueError("collate_batch: T_in = %d, T_out = %d do not cover the batch (%d symbols, %d frames)"
                         % (T_in, T_out, need_in, need_out))
    return indices


COLLATE_OUT = (('text_padded', torch.int64), ('mel_padded', torch.float32), ('gate_padded', torch.float32),
               ('output_lengths', torch.int64), ('speakers', torch.int64), ('emotions', torch.int64))


def collate_batch(store, idx, T_in, T_out, out=None):
    """One launch of t2v_collate_batch on the current stream: rows idx[0 .. B) of the store as the reference's padded batch.
    idx: the utterance indices in row order.  A list or a CPU tensor is checked here (collate_check) and uploaded; a device
    int32 tensor is taken as checked by its maker (corpus.ResidentCollate checks before its asynchronous upload, so this
    path never reads device memory back).  out: the six tensors (text_padded, mel_padded, gate_padded, output_lengths,
    speakers, emotions), contiguous and of the right shapes, instead of fresh torch.empty memory.  Returns the six."""
    lib = _require_gpu(store.mel)
    T_in, T_out = int(T_in), int(T_out)
    if not (torch.is_tensor(idx) and idx.is_cuda):
        idx = torch.tensor(collate_check(store, idx, T_in, T_out), dtype=torch.int32).to(store.mel.device)
    if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != store.mel.device:
        raise T2VHipError("collate_batch: idx must be a contiguous int32 vector on the store's device")
    B = idx.numel()
    shapes = ((B, T_in), (B, 80, T_out), (B, T_out), (B,), (B, store.n_speakers), (B, store.n_emotions))
    if out is None:
        out = tuple(torch.empty(s, dtype=dt, device=idx.device) for s, (_, dt) in zip(shapes, COLLATE_OUT))
    else:
        out = tuple(out)
        if len(out) != len(COLLATE_OUT):
            raise ValueError("collate_batch: out= takes %d tensors" % len(COLLATE_OUT))
        for t, s, (name, dt) in zip(out, shapes, COLLATE_OUT):
            if not t.is_cuda or t.device != idx.device or t.dtype != dt or tuple(t.shape) != s or not t.is_contiguous():
                raise ValueError("collate_batch: out= %s must be a contiguous %s device tensor of shape %s" % (name, dt, s))
    _check(lib.t2v_collate_batch(_p(store.mel), _p(store.mel_off), _p(store.n_frames), _p(store.ids), _p(store.id_off),
                                 _p(store.n_ids), _p(store.speaker), _p(store.emotion), _p(idx), B, store.n_utts, T_in, T_out,
                                 store.n_speakers, store.n_emotions, *([_p(t) for t in out] + [_stream()])),
           't2v_collate_batch')
    return out


def _checked_lengths(v, B, lo, hi, count_msg, range_msg, reject_float=True, reject_bool=True, default=None, dtype=torch.int32):
    """The one check of a lengths argument: B values in lo..hi from a list, a CPU or a device tensor (None: B times `default`, for
    a caller that has one), as a host tensor of `dtype` (None: as it came).  ValueError(count_msg + the values) on a wrong count or
    a rejected element type, ValueError(range_msg + the values) outside the range.  reject_float / reject_bool: each caller's
    acceptance as it has always been; a float that is let in is compared, and converted, truncated."""
    n = torch.full((B,), default, dtype=torch.int64) if v is None and default is not None else torch.as_tensor(v).reshape(-1).cpu()
    if (reject_float and n.dtype.is_floating_point) or (reject_bool and n.dtype == torch.bool) or n.numel() != B:
        raise ValueError("%s, got %s" % (count_msg, n.tolist()))
    if int(n.min()) < lo or int(n.max()) > hi:
        raise ValueError("%s, got %s" % (range_msg, n.tolist()))
    return n if dtype is None else n.to(dtype)


def _frame_counts(n_frames, B, T, device, min_frames=1):
    """per-utterance frame counts as a device int32 vector (all T when None), checked on the host"""
    msg = "every utterance needs %d <= frames <= %d" % (min_frames, T)
    return _checked_lengths(n_frames, B, min_frames, T, msg, msg, reject_float=False, reject_bool=False, default=T).to(device)


def _stft_lengths(n_samples, B, N):
    """stft_polar's sample counts on the host, in the type they came in (all N when None); F.pad(mode='reflect') needs > n_fft/2 each"""
    msg = "stft: every utterance needs 512 < n_samples <= %d" % N
    return _checked_lengths(n_samples, B, 513, N, msg, msg, reject_float=False, reject_bool=False, default=N, dtype=None)


def stft_polar(wav, n_samples, tables, t_stride=None):
    """STFT.transform on device (csrc/vocoder.hip k_stft_polar).  wav: (B,N) float32 CUDA tensor; n_samples: (B) int64
    or None (all N).  tables: window / tw512 / tw1024 device tensors (stft.STFT).  Returns magnitude, phase (B,513,T_max)."""
    lib = _require_gpu(wav)
    B, N = wav.shape
    wav = _f32c(wav)
    n = _stft_lengths(n_samples, B, N)
    if t_stride is None:
        t_stride = int(n.max()) // 256 + 1
    mag = torch.empty(B, 513, t_stride, device=wav.device, dtype=torch.float32)
    phase = torch.empty_like(mag)
    _check(lib.t2v_stft_polar(_p(wav), _p(n.to(wav.device)), B, N, 1024, 256, _p(tables['window']), _p(tables['tw512']),
                              _p(tables['tw1024']), _p(mag), _p(phase), t_stride, _stream()), 't2v_stft_polar')
    return mag, phase


def istft(mag, phase, n_frames, tables):
    """STFT.inverse on device (k_spec_to_frames + k_ola).  mag, phase: (B,513,T) float32 CUDA tensors; n_frames: (B)
    frame counts or None (all T).  Returns (B, (T-1)*256), zero past each utterance's (T_b-1)*256 samples."""
    lib = _require_gpu(mag, phase)
    B, nb, T = mag.shape
    if nb != 513 or phase.shape != mag.shape:
        raise ValueError("istft: magnitude and phase must both be (B, 513, T)")
    mag, phase = _f32c(mag), _f32c(phase)
    n = _frame_counts(n_frames, B, T, mag.device)
    out = torch.empty(B, 256 * (T - 1), device=mag.device, dtype=torch.float32)
    scratch = torch.empty(lib.t2v_istft_scratch_bytes(B, T), device=mag.device, dtype=torch.uint8)
    _check(lib.t2v_istft(_p(mag), _p(phase), _p(n), B, T, 1024, 256, _p(tables['window']), _p(tables['tw512']),
                         _p(tables['tw1024']), _p(scratch), _p(out), out.size(1), _stream()), 't2v_istft')
    return out


def griffin_lim(mag, angles, n_frames, tables, n_iters, momentum=0.0):
    """audio_processing.griffin_lim on device: one inverse from `angles`, n_iters fused iterations (k_gl_iter, one launch
    each, no host synchronisation), final overlap-add.  mag, angles: (B,513,T) float32 CUDA tensors; every utterance needs
    >= 4 frames (the reflect pad of each iteration's transform).  Returns (B, (T-1)*256), zero past each length.
    momentum in (0, 1): fast Griffin-Lim (t2v_griffin_lim_fast, k_gl_iter_fast); 0 is the plain iteration's own entry."""
    momentum = check_momentum(momentum)
    lib = _require_gpu(mag, angles)
    B, nb, T = mag.shape
    if nb != 513 or angles.shape != mag.shape:
        raise ValueError("griffin_lim: magnitudes and angles must both be (B, 513, T)")
    mag, angles = _f32c(mag), _f32c(angles)
    n = _frame_counts(n_frames, B, T, mag.device, min_frames=4)
    out = torch.empty(B, 256 * (T - 1), device=mag.device, dtype=torch.float32)
    if momentum == 0.0:
        scratch = torch.empty(lib.t2v_griffin_lim_scratch_bytes(B, T), device=mag.device, dtype=torch.uint8)
        _check(lib.t2v_griffin_lim(_p(mag), _p(angles), _p(n), B, T, 1024, 256, int(n_iters), _p(tables['window']),
                                   _p(tables['tw512']), _p(tables['tw1024']), _p(scratch), _p(out), out.size(1), _stream()),
               't2v_griffin_lim')
        return out
    scratch = torch.empty(lib.t2v_griffin_lim_fast_scratch_bytes(B, T), device=mag.device, dtype=torch.uint8)
    _check(lib.t2v_griffin_lim_fast(_p(mag), _p(angles), _p(n), B, T, 1024, 256, int(n_iters), momentum,
                                    _p(tables['window']), _p(tables['tw512']), _p(tables['tw1024']), _p(scratch), _p(out),
                                    out.size(1), _stream()), 't2v_griffin_lim_fast')
    return out


def spsi_phase(mag, n_frames=None):
    """A phase for magnitudes alone, on device (csrc/phase_init.hip k_spsi_scan, k_spsi_assign): single-pass spectrogram
    inversion, the start `griffin_lim(init='spsi')` takes instead of a random draw.  mag: (B, 513, T) float32 CUDA tensor as
    `stft_polar` gives it; n_frames: (B) frame counts or None (all T), at least 1 per row; frames at and past a count are not
    read.  Returns the phase (B, 513, T) in [-pi, pi), +0 past each count and in frames without a spectral peak.  Every bin
    follows its frame's nearest peak, whose phase advances by (k + p) / 4 turns per frame, summed in 32-bit fixed point
    (include/t2vae.h): a row gives the same bits alone, in any batch and at any stride."""
    lib = _require_gpu(mag)
    if mag.dim() != 3 or mag.size(1) != 513 or mag.size(0) < 1 or mag.size(2) < 1:
        raise ValueError("spsi_phase: magnitudes must be (B, 513, T), got %s" % (tuple(mag.shape),))
    B, _, T = mag.shape
    if T > TSM_MAX_FRAMES:
        raise ValueError("spsi_phase: rows of %d frames exceed the %d supported" % (T, TSM_MAX_FRAMES))
    mag = _f32c(mag)
    n = _frame_counts(n_frames, B, T, mag.device)
    phase = torch.empty_like(mag)
    scratch = torch.empty(lib.t2v_spsi_scratch_bytes(B, T), device=mag.device, dtype=torch.uint8)
    _check(lib.t2v_spsi(_p(mag), _p(n), B, T, T, _p(phase), _p(scratch), _stream()), 't2v_spsi')
    return phase


def check_momentum(momentum):
    """fast Griffin-Lim's momentum as a float in [0, 1); ValueError otherwise"""
    m = float(momentum)
    if not 0.0 <= m < 1.0:
        raise ValueError("griffin_lim: momentum must be in [0, 1), got %r" % (momentum,))
    return m


def mel_to_magnitude(mel, n_frames, pinv_basis):
    """max(pinv(mel_basis) exp(mel), 0) on device (k_mel_to_mag).  mel: (B,80,T) float32 CUDA tensor; pinv_basis: (513,80)
    device tensor.  Returns (B,513,T), zero past each utterance's frame count."""
    lib = _require_gpu(mel, pinv_basis)
    B, n_mel, T = mel.shape
    mel = _f32c(mel)
    n = _frame_counts(n_frames, B, T, mel.device)
    mag = torch.empty(B, 513, T, device=mel.device, dtype=torch.float32)
    _check(lib.t2v_mel_to_magnitude(_p(mel), _p(_f32c(pinv_basis)), _p(n), B, T, n_mel, _p(mag), _stream()),
           't2v_mel_to_magnitude')
    return mag


def two_tap_basis(mel_basis, device=None):
    """The mel filterbank (80, 513) in the two-tap form of k_mel_to_mag_nnls, with L = ||B||_2^2 (fp64 on the host).  With
    Slaney triangles a bin lies in at most two filters, and those are adjacent: per bin the lower filter `lo` (0..78) and the
    weights w0 = B[lo, k], w1 = B[lo + 1, k]; per filter the range of bins it covers.  The form is checked to reproduce the
    basis exactly; a basis without that structure is a ValueError.  Returns a dict of tensors on `device` (the basis' own
    when None) and the float 'L'."""
    import numpy as np
    B = mel_basis.detach().cpu().float().numpy()
    if B.ndim != 2 or B.shape != (80, 513):
        raise ValueError("two_tap_basis: the mel basis must be (80, 513), got %s" % (tuple(B.shape),))
    if not np.isfinite(B).all() or not B.any():
        raise ValueError("two_tap_basis: the mel basis must be finite and not all zero")
    k = np.arange(513)
    nz = B != 0
    first = np.where(nz.any(0), nz.argmax(0), 0)
    lo = np.minimum(first, 78).astype(np.int32)
    w0, w1 = B[lo, k], B[lo + 1, k]
    start = np.where(nz.any(1), nz.argmax(1), 0).astype(np.int32)
    last = np.where(nz.any(1), 512 - nz[:, ::-1].argmax(1), -1)
    length = (last - start + 1).clip(min=0).astype(np.int32)
    back = np.zeros_like(B)                 # what the kernel multiplies by: filter f takes w0 where lo == f, else w1
    for f in range(80):
        r = slice(int(start[f]), int(start[f] + length[f]))
        back[f, r] = np.where(lo[r] == f, w0[r], w1[r])
    if not np.array_equal(back, B):
        bad = np.argwhere(back != B)[0]
        raise ValueError("two_tap_basis: the mel basis is not a bank of overlapping-by-two filters (every bin in at most two "
                         "adjacent filters); first difference at filter %d, bin %d" % (bad[0], bad[1]))
    dev = mel_basis.device if device is None else device
    t = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in
         (('lo', lo), ('w0', w0), ('w1', w1), ('start', start), ('len', length))}
    t['L'] = float(np.linalg.norm(B.astype(np.float64), 2) ** 2)
    return t


def mel_to_magnitude_nnls(mel, n_frames, mel_basis, pinv_basis, n_iters=100):
    """Non-negative least-squares inverse of the mel filterbank on device (k_mel_to_mag_nnls): from mel_to_magnitude's
    max(pinv exp(mel), 0), n_iters projected-gradient steps M <- max(M - B^T (B M - m) / L, 0) in one launch.  mel: (B,80,T)
    float32 CUDA tensor; mel_basis: the (80, 513) filterbank, or what two_tap_basis made of it (a caller with many calls
    builds that once); pinv_basis: (513,80) device tensor.  Returns (B,513,T), zero past each utterance's frame count;
    n_iters = 0 gives mel_to_magnitude's bits."""
    lib = _require_gpu(mel, pinv_basis)
    if int(n_iters) < 0:
        raise ValueError("mel_to_magnitude_nnls: n_iters must be >= 0, got %r" % (n_iters,))
    B, n_mel, T = mel.shape
    mel = _f32c(mel)
    taps = mel_basis if isinstance(mel_basis, dict) else two_tap_basis(mel_basis, mel.device)
    n = _frame_counts(n_frames, B, T, mel.device)
    mag = torch.empty(B, 513, T, device=mel.device, dtype=torch.float32)
    _check(lib.t2v_mel_to_magnitude_nnls(_p(mel), _p(_f32c(pinv_basis)), _p(taps['lo']), _p(taps['w0']), _p(taps['w1']),
                                         _p(taps['start']), _p(taps['len']), taps['L'], int(n_iters), _p(n), B, T, n_mel,
                                         _p(mag), _stream()), 't2v_mel_to_magnitude_nnls')
    return mag


DTW_MAX_FRAMES = _ABI.define('T2V_DTW_MAX_FRAMES')
DTW_SCRATCH_CAP = 256 << 20             # bytes of scratch one t2v_mel_dtw call may ask of the allocator; larger batches run in groups


def _dtw_lengths(n, B, stride, what):
    """frame counts of mel_dtw as a host list, checked: a list, a CPU tensor or a device int tensor"""
    hi = min(stride, DTW_MAX_FRAMES)
    return _checked_lengths(n, B, 1, hi, "mel_dtw: %s must be %d integer frame counts" % (what, B),
                            "mel_dtw: every %s must be in 1..%d (%d frames stored, at most %d supported)"
                            % (what, hi, stride, DTW_MAX_FRAMES), reject_bool=False)


def mel_dtw(x, nx, y, ny):
    """Mel-spectral distortion with dynamic time warping (csrc/dtw.hip k_mel_dtw): x (B,80,Sx), y (B,80,Sy) float32 CUDA
    tensors, pair b compared on its first nx[b] / ny[b] frames (lists, CPU tensors or device int tensors); nothing past a
    length is read.  Local cost: the Euclidean distance of two frames; recurrence: symmetric2 without a band; returns
    D(nx, ny) / (nx + ny) as a (B,) float32 device tensor.  A pair gives the same bits alone and in any batch.  Batches whose
    scratch would exceed DTW_SCRATCH_CAP run in groups."""
    lib = _require_gpu(x, y)
    if x.dim() != 3 or y.dim() != 3 or x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("mel_dtw: x and y must be float32 (B, 80, T) tensors")
    B, n_mel, sx = x.shape
    if y.size(0) != B or B < 1:
        raise ValueError("mel_dtw: %d sequences in x, %d in y" % (B, y.size(0)))
    if n_mel != 80 or y.size(1) != 80:
        raise ValueError("mel_dtw: 80 mel channels only, got %d and %d" % (n_mel, y.size(1)))
    sy = y.size(2)
    if sx < 1 or sy < 1:
        raise ValueError("mel_dtw: empty time axis")
    nx = _dtw_lengths(nx, B, sx, 'nx').to(x.device)
    ny = _dtw_lengths(ny, B, sy, 'ny').to(x.device)
    x, y = _f32c(x), _f32c(y)
    dist = torch.empty(B, device=x.device, dtype=torch.float32)
    per_pair = lib.t2v_mel_dtw_scratch_bytes(1, sx, sy)
    group = max(1, min(B, DTW_SCRATCH_CAP // per_pair))
    for b0 in range(0, B, group):
        nb = min(group, B - b0)
        scratch = torch.empty(lib.t2v_mel_dtw_scratch_bytes(nb, sx, sy), device=x.device, dtype=torch.uint8)
        _check(lib.t2v_mel_dtw(_p(x[b0:]), _p(nx[b0:]), sx, _p(y[b0:]), _p(ny[b0:]), sy, nb, n_mel, _p(dist[b0:]), _p(scratch),
                               _stream()), 't2v_mel_dtw')
    return dist


NCEP = _ABI.define('T2V_NCEP')
CEP_DTW_SCRATCH_CAP = 256 << 20         # bytes of decision table one t2v_cep_dtw_path call may ask of the allocator; larger batches run in groups
ALIGNED_COUNTS = ('n_points', 'n_both', 'n_vde', 'n_gpe')
ALIGNED_SUMS = ('sum_d', 'sum_e', 'sum_e2', 's_xx', 's_yy', 's_xy', 'sum_warp')
_CEP_TABLE = {}                         # 'host' -> the fp32 table, device -> its copy there


def cepstrum_table(device=None):
    """The (13, 80) table of mel_cepstrum: row k - 1 holds sqrt(2 / 80) cos(pi k (n + 1/2) / 80), k = 1..13, made in fp64 with
    numpy and rounded to fp32 once.  device None: the read-only host array; else its cached copy on that device."""
    import numpy as np
    host = _CEP_TABLE.get('host')
    if host is None:
        k = np.arange(1, NCEP + 1, dtype=np.float64)[:, None]
        n = np.arange(80, dtype=np.float64)[None, :]
        host = (np.sqrt(2.0 / 80.0) * np.cos(np.pi * k * (n + 0.5) / 80.0)).astype(np.float32)
        host.setflags(write=False)
        _CEP_TABLE['host'] = host
    if device is None:
        return host
    key = str(torch.device(device))
    if key not in _CEP_TABLE:
        _CEP_TABLE[key] = torch.from_numpy(host.copy()).to(device)
    return _CEP_TABLE[key]


def mel_cepstrum(mels, lengths):
    """Mel cepstrum of log-mels (csrc/aligned.hip k_mel_cepstrum): mels (B, 80, T) float32 CUDA tensor, row b of lengths[b]
    frames (a list, a CPU tensor or a device int tensor); nothing past a length is read.  Returns (B, 13, T) float32:
    c_k(t) = sqrt(2 / 80) sum_n mels[n, t] cos(pi k (n + 1/2) / 80) for k = 1..13 at row k - 1 (c_0 is left out), 0 past each
    length.  This is the cepstrum "from an 80-band log-mel" of the prosody-transfer papers' MCD-13, not a vocoder's
    mel-generalised cepstrum.  A row gives the same bits alone, in any batch and at any stride."""
    lib = _require_gpu(mels)
    if mels.dim() != 3 or mels.dtype != torch.float32:
        raise ValueError("mel_cepstrum: mels must be a float32 (B, 80, T) tensor")
    B, n_mel, T = mels.shape
    if n_mel != 80:
        raise ValueError("mel_cepstrum: 80 mel channels only, got %d" % n_mel)
    if B < 1 or T < 1:
        raise ValueError("mel_cepstrum: empty input %s" % (tuple(mels.shape),))
    n = _checked_lengths(lengths, B, 1, T, "mel_cepstrum: lengths must be %d integer frame counts" % B,
                         "mel_cepstrum: every length must be in 1..%d (frames stored per row)" % T, reject_bool=False)
    mels = _f32c(mels)
    n = n.to(mels.device)
    table = cepstrum_table(mels.device)
    out = torch.empty(B, NCEP, T, device=mels.device, dtype=torch.float32)
    for b0 in range(0, B, 65535):           # the batch is the grid's second dimension
        _check(lib.t2v_mel_cepstrum(_p(mels[b0:]), _p(n[b0:]), T, min(65535, B - b0), n_mel, NCEP, _p(table), _p(out[b0:]), T,
                                    _stream()), 't2v_mel_cepstrum')
    return out


class AlignedScores(collections.namedtuple('AlignedScores', 'dist n_points counts sums path')):
    """What aligned_scores() returns.  dist (B,) float32: D(Tx-1, Ty-1) / (Tx + Ty); n_points (B,) int32: K, the points of the
    warping path; counts (B, 4) int32 with the columns ALIGNED_COUNTS; sums (B, 8) float32 with the columns ALIGNED_SUMS and one
    reserved word; path (B, Kmax, 2) int32 with (i_p, j_p) for p < n_points[b] (undefined past that), or None when it was not
    asked for.  Every column of counts and sums is also an attribute (r.n_gpe: (B,) int32, r.sum_d: (B,) float32)."""
    __slots__ = ()

    def __getattr__(self, name):
        if name in ALIGNED_COUNTS:
            return self.counts[:, ALIGNED_COUNTS.index(name)]
        if name in ALIGNED_SUMS:
            return self.sums[:, ALIGNED_SUMS.index(name)]
        raise AttributeError(name)


def _aligned_lengths(n, B, stride, what):
    """frame counts of aligned_scores as a host tensor, checked as mel_dtw's: a list, a CPU tensor or a device int tensor"""
    hi = min(stride, DTW_MAX_FRAMES)
    return _checked_lengths(n, B, 1, hi, "aligned_scores: %s must be %d integer frame counts" % (what, B),
                            "aligned_scores: every %s must be in 1..%d (%d frames stored, at most %d supported)"
                            % (what, hi, stride, DTW_MAX_FRAMES), reject_bool=False)


def _aligned_track(f, B, n, what):
    """an F0 track of aligned_scores: None, or a float32 (B, S) CUDA tensor that holds every row's frames"""
    if f is None:
        return None, 1
    if not torch.is_tensor(f) or f.dim() != 2 or f.dtype != torch.float32 or f.size(0) != B or f.size(1) < 1:
        raise ValueError("aligned_scores: %s must be a float32 (%d, frames) tensor" % (what, B))
    if int(n.max()) > f.size(1):
        raise ValueError("aligned_scores: %s holds %d frames per row, the lengths ask for %d" % (what, f.size(1), int(n.max())))
    return _f32c(f), f.size(1)


def aligned_scores(cx, nx, cy, ny, f0x=None, f0y=None, return_path=False):
    """The warping path between two cepstra and the scores along it (csrc/aligned.hip k_cep_dtw_fwd, k_cep_dtw_back,
    k_path_scores): cx (B, 13, Sx), cy (B, 13, Sy) float32 CUDA tensors (mel_cepstrum), pair b compared on its first nx[b] /
    ny[b] frames (lists, CPU tensors or device int tensors); nothing past a length is read.  Local cost: the Euclidean distance
    of two frames; recurrence: mel_dtw's (symmetric2, no band), ties to the diagonal, then (i-1, j), then (i, j-1).  f0x
    (B, >= max nx) and f0y (B, >= max ny): F0 tracks in Hz per frame, 0 where unvoiced (t2v_hip.f0); a missing track counts as
    unvoiced everywhere.  Returns an AlignedScores; evaluation.aligned_fields turns one row of its counts and sums into
    mcd_db, vde, gpe, ffe, the log-F0 errors and warp_dev.  With return_path also path (B, max K, 2) int32.  A pair gives the
    same bits alone and in any batch.  Batches whose decision tables would exceed CEP_DTW_SCRATCH_CAP run in groups."""
    lib = _require_gpu(cx, cy, f0x, f0y)
    if cx.dim() != 3 or cy.dim() != 3 or cx.dtype != torch.float32 or cy.dtype != torch.float32:
        raise ValueError("aligned_scores: cx and cy must be float32 (B, 13, T) tensors")
    B, n_cep, sx = cx.shape
    if cy.size(0) != B or B < 1:
        raise ValueError("aligned_scores: %d sequences in cx, %d in cy" % (B, cy.size(0)))
    if n_cep != NCEP or cy.size(1) != NCEP:
        raise ValueError("aligned_scores: %d cepstral coefficients only, got %d and %d" % (NCEP, n_cep, cy.size(1)))
    sy = cy.size(2)
    if sx < 1 or sy < 1:
        raise ValueError("aligned_scores: empty time axis")
    nx_h, ny_h = _aligned_lengths(nx, B, sx, 'nx'), _aligned_lengths(ny, B, sy, 'ny')
    f0x, fsx = _aligned_track(f0x, B, nx_h, 'f0x')
    f0y, fsy = _aligned_track(f0y, B, ny_h, 'f0y')
    dev = cx.device
    nx, ny = nx_h.to(dev), ny_h.to(dev)
    cx, cy = _f32c(cx), _f32c(cy)
    kmax = int((nx_h + ny_h).max()) - 1
    dist = torch.empty(B, device=dev, dtype=torch.float32)
    K = torch.empty(B, device=dev, dtype=torch.int32)
    path = torch.empty(B, kmax, 2, device=dev, dtype=torch.int32)
    counts = torch.empty(B, len(ALIGNED_COUNTS), device=dev, dtype=torch.int32)
    sums = torch.empty(B, len(ALIGNED_SUMS) + 1, device=dev, dtype=torch.float32)
    per_pair = lib.t2v_cep_dtw_scratch_bytes(1, sx, sy)
    group = max(1, min(B, CEP_DTW_SCRATCH_CAP // per_pair))
    for b0 in range(0, B, group):
        nb = min(group, B - b0)
        scratch = torch.empty(lib.t2v_cep_dtw_scratch_bytes(nb, sx, sy), device=dev, dtype=torch.uint8)
        _check(lib.t2v_cep_dtw_path(_p(cx[b0:]), _p(nx[b0:]), sx, _p(cy[b0:]), _p(ny[b0:]), sy, nb, n_cep, _p(dist[b0:]), _p(K[b0:]),
                                    _p(path[b0:]), kmax, _p(scratch), _stream()), 't2v_cep_dtw_path')
    _check(lib.t2v_path_scores(_p(path), _p(K), kmax, _p(cx), _p(nx), sx, _p(cy), _p(ny), sy, _p(f0x), fsx, _p(f0y), fsy, B, n_cep,
                               _p(counts), _p(sums), _stream()), 't2v_path_scores')
    return AlignedScores(dist, K, counts, sums, path if return_path else None)


F0_MAX_LAG = _ABI.define('T2V_F0_MAX_LAG')
F0_SAMPLE_RATE = 16000                  # the tracker's geometry is the front end's: 16 kHz, hop 256, window 1024
F0_HOP = 256


def f0_lags(fmin=60.0, fmax=500.0):
    """(tau_min, tau_max) of f0(): floor(16000 / fmax), ceil(16000 / fmin); ValueError outside 40 <= fmin < fmax <= 1000"""
    fmin, fmax = float(fmin), float(fmax)
    if not 40.0 <= fmin < fmax <= 1000.0:
        raise ValueError("f0: fmin %g, fmax %g; 40 <= fmin < fmax <= 1000 Hz is supported" % (fmin, fmax))
    tau_min, tau_max = int(math.floor(F0_SAMPLE_RATE / fmax)), int(math.ceil(F0_SAMPLE_RATE / fmin))
    if not 1 <= tau_min < tau_max <= F0_MAX_LAG:
        raise ValueError("f0: fmin %g, fmax %g give the lags %d..%d; 1 <= tau_min < tau_max <= %d is supported"
                         % (fmin, fmax, tau_min, tau_max, F0_MAX_LAG))
    return tau_min, tau_max


def _f0_lengths(lengths, B, S):
    """sample counts of f0() as a host int32 tensor, checked: a list, a CPU tensor or a device int tensor"""
    return _checked_lengths(lengths, B, 1, S, "f0: lengths must be %d integer sample counts" % B,
                            "f0: every length must be in 1..%d (samples stored per row)" % S)


def f0(y, lengths, fmin=60.0, fmax=500.0, threshold=0.1, return_aperiodicity=False):
    """YIN pitch tracks (csrc/f0.hip k_f0_yin): y (B, S) float32 CUDA tensor of 16 kHz waveforms, row b of lengths[b] samples
    (a list, a CPU tensor or a device int tensor); samples outside a row's length count as 0 and are not read.  Frames as
    the mel front end's: hop 256, lengths[b] // 256 + 1 of them, integration window 1024, lags floor(16000 / fmax) ..
    ceil(16000 / fmin).  Returns f0 (B, max frame count) float32 in Hz, 0 where a frame is unvoiced (no lag with
    d' < threshold) or past the row's frame count; with return_aperiodicity also d' at the chosen lag (1 where unvoiced or
    past the end).  A row gives the same bits alone, in any batch and at any stride."""
    lib = _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("f0: y must be a float32 (B, S) tensor, got %s %s" % (y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("f0: empty input %s" % (tuple(y.shape),))
    tau_min, tau_max = f0_lags(fmin, fmax)
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise ValueError("f0: threshold %g must lie in (0, 1)" % threshold)
    n = _f0_lengths(lengths, B, S)
    T = int(n.max()) // F0_HOP + 1
    stride = S // F0_HOP + 1
    y = _f32c(y)
    hz = torch.empty(B, stride, device=y.device, dtype=torch.float32)
    ap = torch.empty(B, stride, device=y.device, dtype=torch.float32)
    _check(lib.t2v_f0_yin(_p(y), _p(n.to(y.device)), S, B, tau_min, tau_max, threshold, _p(hz), _p(ap), stride,
                          _stream()), 't2v_f0_yin')
    if T < stride:
        hz, ap = hz[:, :T].contiguous(), ap[:, :T].contiguous()
    return (hz, ap) if return_aperiodicity else hz


RESAMPLE_MAX_TAPS = _ABI.define('T2V_RESAMPLE_MAX_TAPS')
TRIM_HOP = 256                          # the trim's frames are the front end's: hop 256, window 1024
_RESAMPLE_TAPS = {}                     # (up, down, zeros, beta, rolloff) -> (half, host taps, {device: device taps})


def resample_ratio(sr_in, sr_out):
    """(up, down) of sr_in -> sr_out in lowest terms; ValueError unless both are positive integers"""
    if isinstance(sr_in, bool) or isinstance(sr_out, bool) or int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError("resample: the rates must be positive integers, got %r -> %r" % (sr_in, sr_out))
    sr_in, sr_out = int(sr_in), int(sr_out)
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def resample_length(n, up, down):
    """ceil(n up / down): the samples t2v_resample gives for n"""
    return -((-int(n) * up) // down)


def resample_taps(sr_in, sr_out, zeros=16, beta=8.6, rolloff=0.95):
    """(up, down, half, taps) of resample(): the ratio in lowest terms and the Kaiser-windowed sinc t[0 .. 2 half] = up g, with
    g[k] = fc sinc(fc (k - half)) kaiser_beta(k) normalised to sum 1, half = zeros max(up, down), fc = rolloff / max(up, down),
    made in fp64 with numpy and rounded to fp32 once (a read-only host array, cached per argument tuple).  g is the `window`
    with which scipy.signal.resample_poly(x, up, down) computes the same outputs.  ValueError, naming the ratio, when the
    table would exceed RESAMPLE_MAX_TAPS entries."""
    import numpy as np
    up, down = resample_ratio(sr_in, sr_out)
    zeros, beta, rolloff = int(zeros), float(beta), float(rolloff)
    if zeros < 1 or beta < 0.0 or not 0.0 < rolloff <= 1.0:
        raise ValueError("resample_taps: zeros %r >= 1, beta %r >= 0 and 0 < rolloff %r <= 1 are supported" % (zeros, beta, rolloff))
    key = (up, down, zeros, beta, rolloff)
    hit = _RESAMPLE_TAPS.get(key)
    if hit is None:
        half = zeros * max(up, down)
        if 2 * half + 1 > RESAMPLE_MAX_TAPS:
            raise ValueError("resample: %d -> %d Hz is the ratio %d/%d, whose table of %d taps exceeds the %d supported"
                             % (sr_in, sr_out, up, down, 2 * half + 1, RESAMPLE_MAX_TAPS))
        fc = rolloff / max(up, down)
        k = np.arange(2 * half + 1, dtype=np.float64)
        g = fc * np.sinc(fc * (k - half)) * np.kaiser(2 * half + 1, beta)
        g /= g.sum()
        taps = (up * g).astype(np.float32)
        taps.setflags(write=False)
        hit = _RESAMPLE_TAPS[key] = (half, taps, {})
    return up, down, hit[0], hit[1]


def _wave_lengths(lengths, B, S, who):
    return _checked_lengths(lengths, B, 1, S, "%s: lengths must be %d integer sample counts" % (who, B),
                            "%s: every length must be in 1..%d (samples stored per row)" % (who, S))


def resample(x, lengths, sr_in, sr_out):
    """Polyphase resampling sr_in -> sr_out (csrc/resample.hip k_resample): x (B, S) float32 in [-1, 1) or int16 PCM (scaled by
    1 / 32768 as it is loaded) CUDA tensor, row b of lengths[b] samples (a list, a CPU tensor or a device int tensor); samples
    outside a row's length count as 0 and are not read.  Returns (y (B, max n_out) float32, n_out: the host list of
    ceil(lengths[b] up / down)); y is 0 past each n_out.  What is computed is `resample_taps`' filter applied as
    scipy.signal.resample_poly does.  Equal rates launch nothing: float32 comes back as it is, int16 scaled.  A row gives
    the same bits alone, in any batch and at any stride."""
    lib = _require_gpu(x)
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.int16):
        raise ValueError("resample: x must be a float32 or int16 (B, S) tensor, got %s %s" % (x.dtype, tuple(x.shape)))
    B, S = x.shape
    if B < 1 or S < 1:
        raise ValueError("resample: empty input %s" % (tuple(x.shape),))
    up, down, half, taps = resample_taps(sr_in, sr_out)
    n = _wave_lengths(lengths, B, S, "resample")
    if up == down:
        return (x.contiguous() if x.dtype == torch.float32 else x.float() * (1.0 / 32768.0)), n.tolist()
    n_out = [resample_length(k, up, down) for k in n.tolist()]
    stride = resample_length(S, up, down)
    if S > (1 << 30) or stride > (1 << 30):
        raise ValueError("resample: rows of %d samples (%d after resampling) exceed the 2^30 supported" % (S, stride))
    dev_taps = _RESAMPLE_TAPS[(up, down, 16, 8.6, 0.95)][2]
    t = dev_taps.get(x.device)
    if t is None:
        t = dev_taps[x.device] = torch.from_numpy(taps.copy()).to(x.device)
    x = x.contiguous()
    y = torch.empty(B, stride, device=x.device, dtype=torch.float32)
    _check(lib.t2v_resample(_p(x), int(x.dtype == torch.int16), 1.0 / 32768.0, _p(n.to(x.device)), S, B, _p(t), up, down, half,
                            _p(y), stride, _stream()), 't2v_resample')
    if max(n_out) < stride:
        y = y[:, :max(n_out)].contiguous()
    return y, n_out


TSM_MAX_RATIO = _ABI.define('T2V_TSM_MAX_RATIO')      # the largest numerator and denominator of a rate
TSM_MAX_FRAMES = _ABI.define('T2V_TSM_MAX_FRAMES')
TSM_HOP = 256                           # the STFT's hop, a quarter of its window
_TSM_TABLES = {}                        # device -> the STFT tables of time_stretch


def _small_ratio(x):
    """x > 0 as a fractions.Fraction with numerator and denominator in 1..TSM_MAX_RATIO: limit_denominator on x, or on 1 / x
    where x's own numerator would come out larger"""
    import fractions
    f = fractions.Fraction(x if isinstance(x, (int, fractions.Fraction)) else float(x))
    g = f.limit_denominator(TSM_MAX_RATIO)
    if g.numerator > TSM_MAX_RATIO:
        g = 1 / (1 / f).limit_denominator(TSM_MAX_RATIO)
    return g


def stretch_ratio(rate):
    """(num, den) of a tempo rate (above 1: faster), both in 1..1023: fractions.Fraction(rate).limit_denominator(1023).
    ValueError unless 0.25 <= rate <= 4."""
    try:
        ok = not isinstance(rate, bool) and 0.25 <= rate <= 4.0
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("stretch_ratio: the rate must be a number in 0.25..4, got %r" % (rate,))
    g = _small_ratio(rate)
    return g.numerator, g.denominator


def pitch_ratio(semitones):
    """(p, q) with p / q the frequency factor 2^(semitones / 12), both in 1..1023.  ValueError outside +-12 semitones."""
    try:
        ok = not isinstance(semitones, bool) and -12.0 <= semitones <= 12.0
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("pitch_ratio: the shift must be a number of semitones in -12..12, got %r" % (semitones,))
    g = _small_ratio(2.0 ** (float(semitones) / 12.0))
    return g.numerator, g.denominator


def vocoder_rates(speed, pitch):
    """((num, den), (p, q)) of GriffinLimVocoder(speed=, pitch=): p / q = 2^(pitch / 12), and num / den = speed q / p, the rate
    at which the magnitudes are stretched so that resampling by p / q leaves the duration at 1 / speed.  ValueError when the
    combined rate leaves 0.25..4."""
    import fractions
    p, q = pitch_ratio(pitch)
    sn, sd = stretch_ratio(speed)
    f = fractions.Fraction(sn * q, sd * p)
    if not 0.25 <= f <= 4:
        raise ValueError("speed %r with pitch %r stretches the spectrogram by %s, outside 0.25..4" % (speed, pitch, f))
    g = _small_ratio(f)
    return (g.numerator, g.denominator), (p, q)


def vocoder_warp(pitch, formant=0.0, preserve_formants=False):
    """(a, b) of the one `warp_envelope` call of GriffinLimVocoder(pitch=, formant=, preserve_formants=): the envelope is read at
    k a / b.  With p / q = 2^(pitch / 12) and P / Q = 2^(formant / 12), a / b = (p / q when preserving, else 1) x Q / P: the
    correction that undoes what the resampler will do to the envelope, and the formant factor, as one ratio in 1..1023 each.
    (1, 1) when neither is asked for.  ValueError when the combined ratio leaves 0.25..4."""
    import fractions
    p, q = pitch_ratio(pitch) if preserve_formants else (1, 1)
    P, Q = pitch_ratio(formant)
    f = fractions.Fraction(p * Q, q * P)
    if not 0.25 <= f <= 4:
        raise ValueError("pitch %r (formants preserved) with formant %r warps the envelope by %s, outside 0.25..4" % (pitch, formant, f))
    g = _small_ratio(f)
    return g.numerator, g.denominator


def _rate_pair(rate, who):
    """a rate argument as (num, den): a number goes through stretch_ratio, a pair of integers in 1..1023 is taken as it is"""
    if isinstance(rate, (tuple, list)):
        if len(rate) != 2 or any(isinstance(v, bool) or int(v) != v or not 1 <= v <= TSM_MAX_RATIO for v in rate):
            raise ValueError("%s: a rate given as a pair must be two integers in 1..%d, got %r" % (who, TSM_MAX_RATIO, rate))
        return int(rate[0]), int(rate[1])
    return stretch_ratio(rate)


def stretch_frames(n, num, den):
    """ceil(n den / num): the frames t2v_phase_vocoder gives for n at the rate num / den"""
    return -((-int(n) * den) // num)


def _tsm_launch(who, mag, phase, n_frames, rate, phase_lock):
    lib = _require_gpu(mag) if phase is None else _require_gpu(mag, phase)
    if mag.dim() != 3 or mag.size(1) != 513 or mag.dtype != torch.float32 or (phase is not None and (
            phase.shape != mag.shape or phase.dtype != torch.float32)):
        raise ValueError("%s: magnitude%s must be float32 (B, 513, T)" % (who, "" if phase is None else " and phase"))
    B, _, stride = mag.shape
    if B < 1 or stride < 1:
        raise ValueError("%s: empty input %s" % (who, tuple(mag.shape)))
    num, den = _rate_pair(rate, who)
    msg = "%s: every row needs 1 <= frames <= %d" % (who, stride)
    n = _checked_lengths(n_frames, B, 1, stride, msg, msg, reject_float=False, reject_bool=False, default=stride)
    T = int(n.max())
    if T > TSM_MAX_FRAMES:
        raise ValueError("%s: rows of %d frames exceed the %d supported" % (who, T, TSM_MAX_FRAMES))
    n_out = [stretch_frames(k, num, den) for k in n.tolist()]
    out_stride = max(n_out)
    mag = mag.contiguous()
    mag_out = torch.empty(B, 513, out_stride, device=mag.device, dtype=torch.float32)
    phase_out = scratch = None
    if phase is not None:
        phase = phase.contiguous()
        phase_out = torch.empty_like(mag_out)
        if phase_lock:
            scratch = torch.empty(int(lib.t2v_phase_vocoder_scratch_bytes(B, out_stride, 1)), device=mag.device, dtype=torch.uint8)
    _check(lib.t2v_phase_vocoder(_p(mag), None if phase is None else _p(phase), _p(n.to(mag.device)), B, T, stride, num, den,
                                 int(bool(phase_lock)), _p(mag_out), None if phase is None else _p(phase_out), out_stride,
                                 None if scratch is None else _p(scratch), _stream()), 't2v_phase_vocoder')
    return mag_out, phase_out, n_out


def phase_vocoder(mag, phase, n_frames, rate, phase_lock=True):
    """Time-scale modification of polar spectrograms (csrc/tsm.hip k_pv_scan, k_pv_lock): mag, phase (B, 513, T) float32 CUDA
    tensors as `stft_polar` gives them, row b of n_frames[b] frames (a list, a CPU or a device tensor; None: all T); frames at
    and past a row's count are not read.  rate: a number in 0.25..4 (`stretch_ratio`; above 1 is faster) or a pair (num, den).
    Returns (mag_out, phase_out (B, 513, max n_out), n_out: the host list of ceil(n_frames[b] den / num)), both 0 past each
    n_out.  What is computed is librosa.effects.time_stretch's phase vocoder with exact frame positions (include/t2vae.h); the
    phases come modulo 2 pi, from a prefix sum in 32-bit fixed point.  phase_lock: identity phase locking to the peaks of each
    analysis frame.  A row gives the same bits alone, in any batch and at any stride."""
    return _tsm_launch("phase_vocoder", mag, phase, n_frames, rate, phase_lock)


def stretch_magnitude(mag, n_frames, rate):
    """The magnitude half of `phase_vocoder` alone, for a caller that makes its own phases (Griffin-Lim): returns
    (mag_out (B, 513, max n_out), n_out)."""
    mag_out, _, n_out = _tsm_launch("stretch_magnitude", mag, None, n_frames, rate, False)
    return mag_out, n_out


def _tsm_tables(device):
    t = _TSM_TABLES.get(device)
    if t is None:
        from stft import fft_tables
        t = _TSM_TABLES[device] = {k: torch.from_numpy(v).to(device) for k, v in fft_tables(1024).items()}
    return t


ENV_MAX_ORDER = _ABI.define('T2V_ENV_MAX_ORDER')      # the longest lifter, in cepstral bins
ENV_MAX_ITERS = _ABI.define('T2V_ENV_MAX_ITERS')      # the most true-envelope iterations


def _envelope_launch(who, mag, n_frames, order, iters, ratio, want_env, want_mag):
    """one t2v_spectral_envelope call: (the log envelope or None, the warped magnitudes or None)"""
    lib = _require_gpu(mag)
    if mag.dim() != 3 or mag.size(1) != 513 or mag.dtype != torch.float32:
        raise ValueError("%s: magnitude must be float32 (B, 513, T)" % who)
    B, _, stride = mag.shape
    if B < 1 or stride < 1:
        raise ValueError("%s: empty input %s" % (who, tuple(mag.shape)))
    if isinstance(order, bool) or int(order) != order or not 1 <= order <= ENV_MAX_ORDER:
        raise ValueError("%s: order %r must be an integer in 1..%d" % (who, order, ENV_MAX_ORDER))
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= iters <= ENV_MAX_ITERS:
        raise ValueError("%s: iters %r must be an integer in 0..%d" % (who, iters, ENV_MAX_ITERS))
    if not isinstance(ratio, (tuple, list)):
        raise ValueError("%s: the ratio must be a pair (p, q) of integers in 1..%d, got %r" % (who, TSM_MAX_RATIO, ratio))
    p, q = _rate_pair(ratio, who)
    msg = "%s: every row needs 1 <= frames <= %d" % (who, stride)
    n = _checked_lengths(n_frames, B, 1, stride, msg, msg, reject_float=False, reject_bool=False, default=stride)
    T = int(n.max())
    if T > TSM_MAX_FRAMES:
        raise ValueError("%s: rows of %d frames exceed the %d supported" % (who, T, TSM_MAX_FRAMES))
    mag = mag.contiguous()
    env = torch.empty_like(mag) if want_env else None
    out = torch.empty_like(mag) if want_mag else None
    _check(lib.t2v_spectral_envelope(_p(mag), _p(n.to(mag.device)), B, T, stride, int(order), int(iters), p, q,
                                     None if env is None else _p(env), None if out is None else _p(out), stride, _stream()),
           't2v_spectral_envelope')
    return env, out


def spectral_envelope(mag, n_frames, order=32, iters=8):
    """The true-envelope estimate of STFT magnitudes (csrc/envelope.hip k_spectral_envelope): mag (B, 513, T) float32 CUDA tensor
    as `stft_polar` gives it, row b of n_frames[b] frames (a list, a CPU or a device tensor; None: all T); frames at and past a
    row's count are not read.  Returns the natural-log envelope (B, 513, T), 0 past each count: `iters` + 1 passes of a cepstral
    lifter of `order` bins (1..256) over max(log magnitude, last envelope), a fixed count in 0..32 (include/t2vae.h); iters = 0
    is the plain cepstral envelope.  The lifter must stay below half the pitch period in samples: 32 serves voices up to 250 Hz
    at 16 kHz.  A frame gives the same bits alone, in any batch and at any stride."""
    return _envelope_launch("spectral_envelope", mag, n_frames, order, iters, (1, 1), True, False)[0]


def warp_envelope(mag, n_frames, ratio, order=32, iters=8):
    """The magnitudes with their envelope read at k p / q: mag[k] exp(Ew[k] - E[k]), E the envelope of `spectral_envelope` and
    Ew[k] its linear interpolation at bin k p / q (bin 512 beyond the end).  ratio is the pair (p, q), integers in 1..1023 as
    `pitch_ratio` gives them: the envelope, and with it the formants, moves along frequency by q / p, and the harmonics stay
    where they are.  Returns (B, 513, T), 0 past each count; p == q returns the magnitudes bit for bit."""
    return _envelope_launch("warp_envelope", mag, n_frames, order, iters, ratio, False, True)[1]


def _stretched(who, y, lengths, rate, phase_lock, warp=None, order=32, iters=8):
    """The whole of `time_stretch`, and the middle it shares with the formant-preserving `pitch_shift`: `stft_polar`,
    `warp_envelope` by `warp` when there is one, `phase_vocoder` at `rate`, `istft`, and the cut to each row's length"""
    _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("%s: y must be a float32 (B, S) tensor, got %s %s" % (who, y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("%s: empty input %s" % (who, tuple(y.shape)))
    num, den = _rate_pair(rate, who)
    n = _wave_lengths(lengths, B, S, who)
    if num == den and warp is None:
        return y, n.tolist()
    tables = _tsm_tables(y.device)
    mag, phase = stft_polar(y, n.to(torch.int64), tables)            # the transform reads 64-bit counts
    frames = [k // TSM_HOP + 1 for k in n.tolist()]
    for b, f in enumerate(frames):
        if stretch_frames(f, num, den) < 2:
            raise ValueError("%s: row %d has %d frames, fewer than 2 at the rate %d/%d" % (who, b, f, num, den))
    if warp is not None:
        mag = warp_envelope(mag, frames, warp, order, iters)
    mag, phase, t_out = phase_vocoder(mag, phase, frames, (num, den), phase_lock)
    y_out = istft(mag, phase, t_out, tables)
    n_out = [min((t - 1) * TSM_HOP, stretch_frames(k, num, den)) for t, k in zip(t_out, n.tolist())]
    # istft is 0 past (t_out - 1) 256 samples; what lies between a row's n_out and that is cut here
    y_out.masked_fill_(torch.arange(y_out.size(1), device=y.device)[None, :] >= torch.tensor(n_out, device=y.device)[:, None], 0.0)
    if max(n_out) < y_out.size(1):
        y_out = y_out[:, :max(n_out)].contiguous()
    return y_out, n_out


def time_stretch(y, lengths, rate, phase_lock=True):
    """Change the tempo of waveforms and keep their pitch: y (B, S) float32 CUDA tensor, row b of lengths[b] samples, every one
    more than 512 (`stft_polar`'s ValueError otherwise).  Exactly `stft_polar` -> `phase_vocoder` -> `istft` with the tables
    of stft.STFT.  Returns (y_out (B, max n_out) float32, n_out: the host list of min((T_out[b] - 1) 256, ceil(lengths[b] den /
    num)), T_out[b] the row's stretched frame count); y_out is 0 past each n_out.  A rate of 1 launches nothing and returns
    the input."""
    return _stretched("time_stretch", y, lengths, rate, phase_lock)


def pitch_shift(y, lengths, semitones, phase_lock=True, preserve_formants=False, order=32, iters=8):
    """Change the pitch of waveforms by `semitones` (-12..12) and keep their duration to within a frame: `time_stretch` by q / p,
    then `resample` by p / q read backwards (p / q = 2^(semitones / 12), `pitch_ratio`).  Returns (y_out, n_out) as `resample`
    does.  0 semitones returns the input.  The resampler moves the spectral envelope with the harmonics, so the plain shift
    changes the timbre too.  preserve_formants: the magnitudes go through `warp_envelope` by (p, q) (a lifter of `order`,
    `iters` iterations) between `stft_polar` and `phase_vocoder`, which moves the envelope by q / p ahead of the resampler:
    F0 moves and the formants stay."""
    p, q = pitch_ratio(semitones)
    if p == q:
        return time_stretch(y, lengths, (1, 1))                         # its checks, no launch
    if not preserve_formants:
        stretched, n = time_stretch(y, lengths, (q, p), phase_lock)
    else:
        stretched, n = _stretched("pitch_shift", y, lengths, (q, p), phase_lock, (p, q), order, iters)
    return resample(stretched, n, p, q)


def formant_shift(y, lengths, semitones, order=32, iters=8):
    """Move the spectral envelope of waveforms, their formants, up by 2^(semitones / 12) (-12..12) and keep harmonics and
    duration: `stft_polar` -> `warp_envelope` by (q, p), p / q = `pitch_ratio`(semitones) -> `istft` with the analysis phases.
    y (B, S) float32 CUDA tensor, row b of lengths[b] samples, every one more than 512.  Returns (y_out (B, max n_out), n_out: the
    host list of (lengths[b] // 256) 256), 0 past each n_out.  0 semitones launches nothing and returns the input."""
    _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("formant_shift: y must be a float32 (B, S) tensor, got %s %s" % (y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("formant_shift: empty input %s" % (tuple(y.shape),))
    p, q = pitch_ratio(semitones)
    n = _wave_lengths(lengths, B, S, "formant_shift")
    if p == q:
        return y, n.tolist()
    tables = _tsm_tables(y.device)
    mag, phase = stft_polar(y, n.to(torch.int64), tables)
    frames = [k // TSM_HOP + 1 for k in n.tolist()]
    mag = warp_envelope(mag, frames, (q, p), order, iters)
    return istft(mag, phase, frames, tables), [(f - 1) * TSM_HOP for f in frames]


def trim_bounds(y, lengths, top_db=40.0, pad_frames=2):
    """Where each row sounds (csrc/resample.hip k_trim_ms, k_trim_bounds): y (B, S) float32 CUDA tensor, row b of lengths[b]
    samples.  Frames as the mel front end's (hop 256, window 1024 centred on 256 t, lengths[b] // 256 + 1 of them); a frame
    sounds when its mean square exceeds the row's loudest frame's by more than -top_db dB.  Returns a device int32 (B, 2)
    tensor of (start, end): 256 max(0, first - pad_frames) and min(lengths[b], 256 (last + 1 + pad_frames)) for the outermost
    sounding frames, (0, lengths[b]) for a row without one (all zeros)."""
    lib = _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("trim_bounds: y must be a float32 (B, S) tensor, got %s %s" % (y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("trim_bounds: empty input %s" % (tuple(y.shape),))
    top_db = float(top_db)
    if not 0.0 < top_db < float('inf'):
        raise ValueError("trim_bounds: top_db %r must be positive and finite" % (top_db,))
    if isinstance(pad_frames, bool) or int(pad_frames) != pad_frames or not 0 <= pad_frames <= (1 << 20):
        raise ValueError("trim_bounds: pad_frames %r must be an integer in 0..2^20" % (pad_frames,))
    n = _wave_lengths(lengths, B, S, "trim_bounds")
    y = _f32c(y)
    stride = S // TRIM_HOP + 1
    ms = torch.empty(B, stride, device=y.device, dtype=torch.float32)
    bounds = torch.empty(B, 2, device=y.device, dtype=torch.int32)
    _check(lib.t2v_trim_bounds(_p(y), _p(n.to(y.device)), S, B, top_db, int(pad_frames), _p(ms), stride, _p(bounds), _stream()),
           't2v_trim_bounds')
    return bounds


def crop(y, bounds, pcm16=False, return_stats=False):
    """Rows cut to their bounds (csrc/resample.hip k_crop_rows): y (B, S) float32 CUDA tensor, bounds (B, 2) integers (start, end)
    with 0 <= start <= end <= S, a device tensor (as trim_bounds gives it), a CPU tensor or a list.  Returns (out, counts): out
    (B, max(end - start)) with y[b, start:end] from column 0 and zeros behind it, counts the host list of end - start.
    pcm16: out is int16, y 32768 rounded to nearest-even and clamped to [-32768, 32767]; with return_stats (pcm16 only) a third
    value, the host list of (clipped samples, max |y|) per row, over [start, end)."""
    lib = _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("crop: y must be a float32 (B, S) tensor, got %s %s" % (y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("crop: empty input %s" % (tuple(y.shape),))
    if return_stats and not pcm16:
        raise ValueError("crop: return_stats counts what the int16 conversion clips: it needs pcm16=True")
    bd = torch.as_tensor(bounds)
    if bd.dtype.is_floating_point or bd.dtype == torch.bool or tuple(bd.shape) != (B, 2):
        raise ValueError("crop: bounds must be (%d, 2) integers, got %s %s" % (B, bd.dtype, tuple(bd.shape)))
    host = bd.cpu().to(torch.int64)
    if int(host.min()) < 0 or int(host.max()) > S or bool((host[:, 0] > host[:, 1]).any()):
        raise ValueError("crop: every row needs 0 <= start <= end <= %d, got %s" % (S, host.tolist()))
    counts = (host[:, 1] - host[:, 0]).tolist()
    width = max(max(counts), 1)
    y = _f32c(y)
    bd = bd.to(device=y.device, dtype=torch.int32).contiguous()
    out = torch.empty(B, width, device=y.device, dtype=torch.int16 if pcm16 else torch.float32)
    stats = torch.empty(B, 2, device=y.device, dtype=torch.int32) if return_stats else None
    _check(lib.t2v_crop_rows(_p(y), S, _p(bd), B, _p(out), int(bool(pcm16)), width, _p(stats), _stream()), 't2v_crop_rows')
    if not return_stats:
        return out, counts
    s = stats.cpu()
    peaks = s[:, 1].contiguous().view(torch.float32).tolist()
    return out, counts, [(int(c), float(p)) for c, p in zip(s[:, 0].tolist(), peaks)]


LOUDNESS_CHUNK = _ABI.define('T2V_LOUDNESS_CHUNK')      # samples per lane of k_loud_filter
LOUDNESS_TILE = _ABI.define('T2V_LOUDNESS_TILE')      # samples per workgroup tile, between which the filter state is scanned
LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE = 8000, 48000
LOUDNESS_OFFSET = -0.691                # BS.1770: a full-scale 997 Hz sine reads -3.01 LUFS
_LOUDNESS_TABLES = {}                   # rate -> (host table, {device: device table})


class Loudness(collections.namedtuple('Loudness', 'integrated ungated momentary_max gated_sum gated_blocks n_blocks frame_ms')):
    """What loudness() gives.  Host lists of one value per row: integrated (LUFS: gated as BS.1770-4 says, -inf for a row
    without a gated block), ungated (LUFS of the whole row's mean square), momentary_max (LUFS of the loudest 400 ms block, -inf
    without one), gated_sum and gated_blocks (the sum of the gated blocks' powers and their count: sum them over rows to pool,
    -0.691 + 10 log10(sum / count)), n_blocks (complete 400 ms blocks); frame_ms (B, max frame count) float32 on the device,
    the K-weighted mean square of the front end's frames, 0 past a row's frame count (energy_db turns it into dB)."""
    __slots__ = ()


def _loudness_rate(sr, who):
    if isinstance(sr, bool) or int(sr) != sr or sr % 10 or not LOUDNESS_MIN_RATE <= sr <= LOUDNESS_MAX_RATE:
        raise ValueError("%s: the rate %r is not supported: a multiple of 10 Hz in %d..%d (100 ms must be whole samples)"
                         % (who, sr, LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE))
    return int(sr)


def kweight_coefficients(sr):
    """The K-weighting of ITU-R BS.1770 at the rate sr, as libebur128 and pyloudnorm derive it, in fp64: the numpy array
    (b0, b1, b2, a1, a2, d1, d2) of the high shelf b / (1, a1, a2) followed by the high pass (1, -2, 1) / (1, d1, d2).  At
    48 000 Hz these are the standard's table.  ValueError, naming the rate, unless sr is a multiple of 10 Hz in 8 000..48 000."""
    import numpy as np
    sr = _loudness_rate(sr, "kweight_coefficients")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return np.array(shelf + [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], dtype=np.float64)


def loudness_table(sr):
    """The fp64 table t2v_loudness takes (include/t2vae.h): the coefficients rounded to fp32 (the six numbers the filter is
    defined by, and the 1 -2 1 of the high pass), and the powers M^0 .. M^64 of M = A^LOUDNESS_CHUNK, A the zero-input step of
    the cascade, computed from the rounded coefficients.  A read-only host array, cached per rate."""
    import numpy as np
    sr = _loudness_rate(sr, "loudness")
    hit = _LOUDNESS_TABLES.get(sr)
    if hit is None:
        c32 = kweight_coefficients(sr).astype(np.float32)
        b0, b1, b2, a1, a2, d1, d2 = c32.astype(np.float64)
        A = np.array([[-a1, 1.0, 0.0, 0.0], [-a2, 0.0, 0.0, 0.0], [-2.0 - d1, 0.0, -d1, 1.0], [1.0 - d2, 0.0, -d2, 0.0]])
        M = np.linalg.matrix_power(A, LOUDNESS_CHUNK)
        table = np.zeros(8 + 16 * 65, dtype=np.float64)
        table[:7] = c32
        P = np.eye(4)
        for p in range(65):
            table[8 + 16 * p:24 + 16 * p] = P.reshape(-1)
            P = M @ P
        table.setflags(write=False)
        hit = _LOUDNESS_TABLES[sr] = (table, {})
    return hit[0]


def energy_db(frame_ms):
    """K-weighted frame level in dB (LUFS scale): -0.691 + 10 log10 max(ms, 1e-12); a tensor, a numpy array or a number"""
    if torch.is_tensor(frame_ms):
        return LOUDNESS_OFFSET + 10.0 * torch.log10(frame_ms.clamp(min=1e-12))
    import numpy as np
    return LOUDNESS_OFFSET + 10.0 * np.log10(np.maximum(np.asarray(frame_ms, dtype=np.float64), 1e-12))


def _lufs(power):
    return LOUDNESS_OFFSET + 10.0 * math.log10(power) if power > 0.0 else float('-inf')


def loudness(y, lengths, sr=16000, return_blocks=False):
    """BS.1770-4 / EBU R 128 loudness and the K-weighted frame energy (csrc/loudness.hip k_loud_filter, k_loud_reduce): y (B, S)
    float32 CUDA tensor of waveforms at the rate sr, row b of lengths[b] samples (a list, a CPU tensor or a device int tensor);
    samples at and past a row's length are not read.  Blocks are 400 ms with a 100 ms hop, complete blocks only; frames are the
    mel front end's (hop 256, window 1024 centred on 256 t, lengths[b] // 256 + 1 of them: the grid of f0() and trim_bounds()).
    Returns a `Loudness`; its per-row scalars come in one device-to-host copy.  With return_blocks also the block powers
    (B, max block count) float32 on the device, 0 past a row's blocks.  A row gives the same bits alone, in any batch and at any
    stride.  ValueError, naming the rate, unless sr is a multiple of 10 Hz in 8 000..48 000."""
    lib = _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("loudness: y must be a float32 (B, S) tensor, got %s %s" % (y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("loudness: empty input %s" % (tuple(y.shape),))
    if S > (1 << 30):
        raise ValueError("loudness: rows of %d samples exceed the 2^30 supported" % S)
    table = loudness_table(sr)
    hop = int(sr) // 10
    n = _wave_lengths(lengths, B, S, "loudness")
    dev_tables = _LOUDNESS_TABLES[int(sr)][1]
    t = dev_tables.get(y.device)
    if t is None:
        t = dev_tables[y.device] = torch.from_numpy(table.copy()).to(y.device)
    y = _f32c(y)
    ms_stride = S // TRIM_HOP + 1
    blk_stride = max((S - 4 * hop) // hop + 1 if S >= 4 * hop else 0, 1)
    ms = torch.empty(B, ms_stride, device=y.device, dtype=torch.float32)
    blocks = torch.empty(B, blk_stride, device=y.device, dtype=torch.float32)
    rows = torch.empty(B, 8, device=y.device, dtype=torch.int32)
    scratch = torch.empty(int(lib.t2v_loudness_scratch_bytes(B, S, hop)), device=y.device, dtype=torch.uint8)
    _check(lib.t2v_loudness(_p(y), _p(n.to(y.device)), S, B, _p(t), hop, _p(ms), ms_stride, _p(blocks), blk_stride, _p(rows),
                            _p(scratch), _stream()), 't2v_loudness')
    r = rows.cpu()
    f = r[:, :3].contiguous().view(torch.float32).double().tolist()
    counts, nb = r[:, 3].tolist(), r[:, 4].tolist()
    T = int(n.max()) // TRIM_HOP + 1
    if T < ms_stride:
        ms = ms[:, :T].contiguous()
    out = Loudness(integrated=[_lufs(g / c) if c else float('-inf') for (g, _, _), c in zip(f, counts)],
                   ungated=[_lufs(u) for _, u, _ in f], momentary_max=[_lufs(m) for _, _, m in f],
                   gated_sum=[g for g, _, _ in f], gated_blocks=counts, n_blocks=nb, frame_ms=ms)
    if not return_blocks:
        return out
    nb_max = max(max(nb), 1)
    return out, (blocks[:, :nb_max].contiguous() if nb_max < blk_stride else blocks)


def scale_rows(y, lengths, gains):
    """y[b, :lengths[b]] *= gains[b] in place (csrc/loudness.hip k_scale_rows): y (B, S) contiguous float32 CUDA tensor, gains B
    numbers (a list, a CPU or a device tensor).  Columns at and past a row's length are untouched.  Returns y."""
    lib = _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("scale_rows: y must be a contiguous float32 (B, S) tensor, got %s %s" % (y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("scale_rows: empty input %s" % (tuple(y.shape),))
    n = _wave_lengths(lengths, B, S, "scale_rows")
    g = torch.as_tensor(gains, dtype=torch.float32).reshape(-1)
    if g.numel() != B:
        raise ValueError("scale_rows: gains must be %d numbers, got %d" % (B, g.numel()))
    g = g.to(y.device).contiguous()
    _check(lib.t2v_scale_rows(_p(y), _p(n.to(y.device)), S, B, _p(g), _stream()), 't2v_scale_rows')
    return y


VOICE_FEATS = ('level_db', 'alpha_db', 'hammarberg_db', 'slope_db_khz', 'cpp_db', 'cpp_lag')      # the planes of t2v_voice_quality, in order
VOICE_FRAMES = _ABI.define('T2V_VOICE_FRAMES')      # frames per workgroup of k_voice_quality
VOICE_SILENT_DB = _ABI.define('T2V_VOICE_SILENT_DB')      # level_db of a frame without energy
VOICE_FLOOR_DB = 40.0                   # a frame is counted within this many dB of the row's loudest frame (the trim's rule)
assert len(VOICE_FEATS) == _ABI.define('T2V_VOICE_FEATS')


class VoiceQuality(collections.namedtuple('VoiceQuality', VOICE_FEATS)):
    """What voice_quality() gives: six (B, max frame count) float32 tracks on the device, +0 past a row's frame count.
    level_db: the 50 Hz - 5 kHz band level, VOICE_SILENT_DB for a frame without energy (`voice_counted` gates on it);
    alpha_db: 1 - 5 kHz over 50 Hz - 1 kHz; hammarberg_db: the peak below 2 kHz over the peak in 2 - 5 kHz; slope_db_khz: the
    spectral slope over 500 - 1500 Hz; cpp_db: the cepstral peak prominence over the 60 - 500 Hz quefrencies; cpp_lag: the
    peak's quefrency in samples.  include/t2vae.h has the definitions."""
    __slots__ = ()


def voice_quality(y, lengths):
    """Spectral balance and cepstral peak prominence per frame (csrc/voice.hip k_voice_quality): y (B, S) float32 CUDA tensor of
    16 kHz waveforms, row b of lengths[b] samples (a list, a CPU tensor or a device int tensor); samples outside a row's length
    count as 0 and are not read.  Frames as the mel front end's (hop 256, window 1024 centred on 256 t, lengths[b] // 256 + 1
    of them: the grid of f0(), loudness() and trim_bounds()).  Returns a `VoiceQuality`.  A row gives the same bits alone, in
    any batch and at any stride."""
    lib = _require_gpu(y)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("voice_quality: y must be a float32 (B, S) tensor, got %s %s" % (y.dtype, tuple(y.shape)))
    B, S = y.shape
    if B < 1 or S < 1:
        raise ValueError("voice_quality: empty input %s" % (tuple(y.shape),))
    if S > (1 << 30):
        raise ValueError("voice_quality: rows of %d samples exceed the 2^30 supported" % S)
    n = _wave_lengths(lengths, B, S, "voice_quality")
    y = _f32c(y)
    stride = S // TRIM_HOP + 1
    out = torch.empty(B, len(VOICE_FEATS), stride, device=y.device, dtype=torch.float32)
    _check(lib.t2v_voice_quality(_p(y), _p(n.to(y.device)), S, B, _p(out), stride, _stream()), 't2v_voice_quality')
    T = int(n.max()) // TRIM_HOP + 1
    return VoiceQuality(*(out[:, k, :T].contiguous() for k in range(len(VOICE_FEATS))))


def voice_counted(level_db, n_frames=None, floor_db=VOICE_FLOOR_DB):
    """The frames of a level_db track that the voice-quality statistics count: not silent, and within floor_db of the row's
    loudest frame.  level_db: a (frames,) or (B, frames) tensor; n_frames: the rows' frame counts where the tensor is wider
    than a row (a list or a tensor), frames at and past them are not counted and do not set the maximum.  Returns a bool
    tensor of level_db's shape; a row without a counted frame (all silent) has none."""
    level = torch.as_tensor(level_db)
    rows = level if level.dim() == 2 else level[None]
    valid = rows > VOICE_SILENT_DB
    if n_frames is not None:
        count = torch.as_tensor(n_frames, device=rows.device).reshape(-1, 1)
        valid = valid & (torch.arange(rows.size(1), device=rows.device)[None, :] < count)
    if rows.size(1) == 0:
        return valid.reshape(level.shape)
    top = rows.masked_fill(~valid, float('-inf')).amax(1, keepdim=True)
    return (valid & (rows > top - floor_db)).reshape(level.shape)


ALIGN_FRAMES = _ABI.define('T2V_ALIGN_FRAMES')      # frames per workgroup of k_align_scan
ALIGN_STATS = ('furthest', 'p_last', 'n_back', 'n_jump', 'longest_stall', 'n_uncovered', 'longest_gap')


class AlignmentStats(collections.namedtuple('AlignmentStats', 'path mass focus stats')):
    """What alignment_stats() returns.  path (B, N) int32, mass (B, T_in) float32, focus (B,) float32, stats (B, 8) int32 with
    the columns ALIGN_STATS and one reserved word; every column of stats is also an attribute (r.n_back: (B,) int32)."""
    __slots__ = ()

    def __getattr__(self, name):
        if name in ALIGN_STATS:
            return self.stats[:, ALIGN_STATS.index(name)]
        raise AttributeError(name)


class _AlignDeviceError(T2VHipError, ValueError):
    """a CPU tensor handed to alignment_stats: a bad argument (ValueError) and, as everywhere here, no CPU path (T2VHipError)"""


def _align_lengths(v, B, hi, what, unit):
    """lengths of alignment_stats as a host int32 tensor, checked: a list, a CPU tensor or a device int tensor"""
    return _checked_lengths(v, B, 1, hi, "alignment_stats: %s must be %d integer %s counts" % (what, B, unit),
                            "alignment_stats: every %s must be in 1..%d (%ss stored per row)" % (what, hi, unit))


def alignment_stats(alignments, n_frames, text_lengths, max_jump=3, cover_min=0.5):
    """Did the decoder read the sentence?  (csrc/align.hip k_align_scan + k_align_finish.)  alignments: (B, N, T_in) float32
    CUDA tensor of attention weights, row b valid on its first n_frames[b] frames and text_lengths[b] text positions (lists,
    CPU tensors or device int tensors); nothing outside is read and the tensor is never written.  The last dimension must have
    stride 1 (another one is a ValueError, not a copy); the other two strides are passed through, so a sliced view of a larger
    tensor works without a copy.  With p[t] = the lowest j that maximises alignments[b, t, j] the AlignmentStats hold
      path  (B, N) int32: p[t], -1 past n_frames[b];      mass (B, T_in) float32: the column sums over the valid frames, 0 past
      text_lengths[b];      focus (B,) float32: the mean of alignments[b, t, p[t]];
      stats (B, 8) int32, columns ALIGN_STATS: furthest (max p), p_last (p of the last frame), n_back (steps p[t] < p[t-1]),
      n_jump (steps p[t] - p[t-1] > max_jump), longest_stall (longest run of equal consecutive p, frames), n_uncovered (text
      positions with mass < cover_min), longest_gap (longest run of consecutive uncovered positions), and a reserved 0.
    A row gives the same bits alone, in any batch, at any stride and with any padding.  max_jump = 3 and cover_min = 0.5 are
    choices, not calibrated against a trained model.
    The teacher-forced `alignments` of `model(x)` fit as they are, with its output_lengths and input_lengths."""
    lib = load_library()
    if not torch.is_tensor(alignments) or alignments.dim() != 3 or alignments.dtype != torch.float32:
        raise ValueError("alignment_stats: alignments must be a float32 (B, N, T_in) tensor, got %s %s"
                         % (getattr(alignments, 'dtype', type(alignments)), tuple(getattr(alignments, 'shape', ()))))
    if not alignments.is_cuda:
        raise _AlignDeviceError("alignment_stats: alignments %s live on %s; this path has no CPU fallback"
                                % (tuple(alignments.shape), alignments.device))
    B, N, T_in = alignments.shape
    if B < 1 or N < 1 or T_in < 1:
        raise ValueError("alignment_stats: empty input %s" % (tuple(alignments.shape),))
    sb, st, sj = alignments.stride()
    if (T_in > 1 and sj != 1) or (N > 1 and st < T_in) or (B > 1 and sb < (N - 1) * st + T_in):
        raise ValueError("alignment_stats: strides %s of shape %s; the last dimension must have stride 1 and rows and frames may "
                         "not overlap" % ((sb, st, sj), (B, N, T_in)))
    st = max(st, T_in) if N == 1 else st              # a dimension of size 1 may report any stride
    sb = max(sb, (N - 1) * st + T_in) if B == 1 else sb
    if isinstance(max_jump, bool) or int(max_jump) != max_jump or max_jump < 0:
        raise ValueError("alignment_stats: max_jump %r must be an integer >= 0" % (max_jump,))
    cover_min = float(cover_min)
    if not cover_min > 0.0 or math.isinf(cover_min):
        raise ValueError("alignment_stats: cover_min %g must be a finite number > 0" % cover_min)
    n = _align_lengths(n_frames, B, N, 'n_frames', 'frame').to(alignments.device)
    L = _align_lengths(text_lengths, B, T_in, 'text_lengths', 'position').to(alignments.device)
    dev = alignments.device
    path = torch.empty(B, N, device=dev, dtype=torch.int32)
    mass = torch.empty(B, T_in, device=dev, dtype=torch.float32)
    focus = torch.empty(B, device=dev, dtype=torch.float32)
    stats = torch.empty(B, 8, device=dev, dtype=torch.int32)
    scratch = torch.empty(lib.t2v_alignment_scratch_bytes(B, N, T_in), device=dev, dtype=torch.uint8)
    _check(lib.t2v_alignment_stats(_p(alignments), sb, st, _p(n), _p(L), B, N, T_in, int(max_jump), cover_min, _p(path), N,
                                   _p(mass), T_in, _p(focus), _p(stats), _p(scratch), _stream()), 't2v_alignment_stats')
    return AlignmentStats(path, mass, focus, stats)


MAS_MAX_SYMBOLS = _ABI.define('T2V_MAS_MAX_SYMBOLS')      # the two live rows of Q sit in LDS
MAS_FLOOR = float(_ABI._macros['T2V_MAS_FLOOR'].rstrip('fF'))      # the header's fp32 literal: a(t, j) = max(A, floor)
MAS_MAX_STEP = 3

MonotonicAlignment = collections.namedtuple('MonotonicAlignment', 'path durations starts score')
MonotonicAlignment.__doc__ = """What mas() returns.  path (B, N) int32, -1 past n_frames[b]; durations (B, T_in) int32, 0 past
n_ids[b]; starts (B, T_in) int32, the prefix sums of durations (0 past n_ids[b]); score (B,) float32, the mean over the row's
frames of ln max(alignments[b, t, path[t]], MAS_FLOOR)."""


def mas_feasible(n_frames, n_ids, max_step=1):
    """whether a monotonic path from symbol 0 at frame 0 to symbol n_ids - 1 at frame n_frames - 1 exists with steps of at most
    max_step symbols per frame (host integers)"""
    return n_frames >= 1 and n_ids >= 1 and n_ids - 1 <= (n_frames - 1) * max_step


def mas(alignments, n_frames, n_ids, max_step=1):
    """Forced alignment by monotonic alignment search (csrc/durations.hip k_mas): the best monotonic path through each
    alignment matrix.  alignments: (B, N, T_in) float32 CUDA tensor of attention weights, row b valid on its first n_frames[b]
    frames and n_ids[b] symbols (lists, CPU tensors or device int tensors); nothing outside is read and the tensor is never
    written.  Strides as `alignment_stats`: the last dimension has stride 1, the other two are passed through.  A path p has
    p[0] = 0, p[n-1] = L - 1 and 0 <= p[t] - p[t-1] <= max_step (1..3; above 1 a symbol may be skipped and gets duration 0);
    the one returned maximises sum_t ln max(alignments[b, t, p[t]], MAS_FLOOR) by the fp32 recurrence of include/t2vae.h, ties
    going to the smaller step.  Returns a MonotonicAlignment.  A row without a feasible path (n_ids - 1 > (n_frames - 1)
    max_step) is a ValueError before anything is launched; T_in above MAS_MAX_SYMBOLS too.  A row gives the same bits alone,
    in any batch, at any stride and with any padding."""
    lib = load_library()
    if not torch.is_tensor(alignments) or alignments.dim() != 3 or alignments.dtype != torch.float32:
        raise ValueError("mas: alignments must be a float32 (B, N, T_in) tensor, got %s %s"
                         % (getattr(alignments, 'dtype', type(alignments)), tuple(getattr(alignments, 'shape', ()))))
    if not alignments.is_cuda:
        raise _AlignDeviceError("mas: alignments %s live on %s; this path has no CPU fallback"
                                % (tuple(alignments.shape), alignments.device))
    B, N, T_in = alignments.shape
    if B < 1 or N < 1 or T_in < 1:
        raise ValueError("mas: empty input %s" % (tuple(alignments.shape),))
    if T_in > MAS_MAX_SYMBOLS:
        raise ValueError("mas: %d symbols per row; at most %d are supported" % (T_in, MAS_MAX_SYMBOLS))
    sb, st, sj = alignments.stride()
    if (T_in > 1 and sj != 1) or (N > 1 and st < T_in) or (B > 1 and sb < (N - 1) * st + T_in):
        raise ValueError("mas: strides %s of shape %s; the last dimension must have stride 1 and rows and frames may not overlap"
                         % ((sb, st, sj), (B, N, T_in)))
    st = max(st, T_in) if N == 1 else st              # a dimension of size 1 may report any stride
    sb = max(sb, (N - 1) * st + T_in) if B == 1 else sb
    if isinstance(max_step, bool) or int(max_step) != max_step or not 1 <= max_step <= MAS_MAX_STEP:
        raise ValueError("mas: max_step %r must be an integer in 1..%d" % (max_step, MAS_MAX_STEP))
    max_step = int(max_step)
    n = _checked_lengths(n_frames, B, 1, N, "mas: n_frames must be %d integer frame counts" % B,
                         "mas: every n_frames must be in 1..%d (frames stored per row)" % N)
    L = _checked_lengths(n_ids, B, 1, T_in, "mas: n_ids must be %d integer symbol counts" % B,
                         "mas: every n_ids must be in 1..%d (symbols stored per row)" % T_in)
    for b, (nb, Lb) in enumerate(zip(n.tolist(), L.tolist())):
        if not mas_feasible(nb, Lb, max_step):
            raise ValueError("mas: row %d has %d symbols and %d frames: no monotonic path with steps <= %d reaches the last "
                             "symbol" % (b, Lb, nb, max_step))
    dev = alignments.device
    n, L = n.to(dev), L.to(dev)
    path = torch.empty(B, N, device=dev, dtype=torch.int32)
    durations = torch.empty(B, T_in, device=dev, dtype=torch.int32)
    starts = torch.empty(B, T_in, device=dev, dtype=torch.int32)
    score = torch.empty(B, device=dev, dtype=torch.float32)
    scratch = torch.empty(lib.t2v_mas_scratch_bytes(B, N, T_in), device=dev, dtype=torch.uint8)
    _check(lib.t2v_mas(_p(alignments), sb, st, _p(n), _p(L), B, N, T_in, max_step, _p(path), N, _p(durations), _p(starts), T_in,
                       _p(score), _p(scratch), _stream()), 't2v_mas')
    return MonotonicAlignment(path, durations, starts, score)


class SegmentMeans(collections.namedtuple('SegmentMeans', 'sums counts')):
    """What segment_means() returns: sums (B, T_in) float32 and counts (B, T_in) int32 per symbol; `means` divides them (NaN
    where a symbol has no counted frame)."""
    __slots__ = ()

    @property
    def means(self):
        return self.sums / self.counts.to(self.sums.dtype)


def segment_means(track, counted, starts, durations):
    """Sums of a frame track over the segments of a monotonic path (csrc/durations.hip k_segment_means).  track: (B, frames)
    float32 CUDA tensor (an F0 or a level track); counted: None (every frame counts) or a bool / uint8 tensor of track's shape;
    starts, durations: (B, T_in) int32 as `mas` returns them.  Symbol j of row b covers the frames [starts, starts + durations),
    clamped to the track; its counted frames are added in ascending frame order.  Returns a SegmentMeans; a segment of
    duration 0, or without a counted frame, has sum 0 and count 0."""
    lib = _require_gpu(track, counted, starts, durations)
    if track.dim() != 2 or track.dtype != torch.float32 or track.size(0) < 1 or track.size(1) < 1:
        raise ValueError("segment_means: track must be a non-empty float32 (B, frames) tensor, got %s %s"
                         % (track.dtype, tuple(track.shape)))
    B, frames = track.shape
    for name, t in (('starts', starts), ('durations', durations)):
        if t.dim() != 2 or t.dtype != torch.int32 or t.size(0) != B or t.size(1) < 1 or t.shape != starts.shape:
            raise ValueError("segment_means: %s must be an int32 (%d, T_in) tensor, got %s %s" % (name, B, t.dtype, tuple(t.shape)))
    if counted is not None:
        if counted.dtype not in (torch.bool, torch.uint8) or counted.shape != track.shape:
            raise ValueError("segment_means: counted must be a bool or uint8 tensor of track's shape %s, got %s %s"
                             % (tuple(track.shape), counted.dtype, tuple(counted.shape)))
        counted = counted.contiguous()
    track, starts, durations = track.contiguous(), starts.contiguous(), durations.contiguous()
    T_in = starts.size(1)
    sums = torch.empty(B, T_in, device=track.device, dtype=torch.float32)
    counts = torch.empty(B, T_in, device=track.device, dtype=torch.int32)
    _check(lib.t2v_segment_means(_p(track), _p(counted), frames, _p(starts), _p(durations), T_in, B, T_in, _p(sums), _p(counts),
                                 T_in, _stream()), 't2v_segment_means')
    return SegmentMeans(sums, counts)


TSNE_MAX_POINTS = _ABI.define('T2V_TSNE_MAX_POINTS')      # P is dense fp32, 1 GiB there
TSNE_MAX_DIM = 64
TSNE_EXAG_ITERS = _ABI.define('T2V_TSNE_EXAG_ITERS')
TSNE_KL_EVERY = 50


def _tsne_check(what, N, D=None, perplexity=None):
    if N < 4 or N > TSNE_MAX_POINTS:
        raise ValueError("%s: %d points; 4..%d are supported (P is a dense N x N fp32 matrix)" % (what, N, TSNE_MAX_POINTS))
    if D is not None and (D < 2 or D > TSNE_MAX_DIM):
        raise ValueError("%s: %d input dimensions; 2..%d are supported" % (what, D, TSNE_MAX_DIM))
    if perplexity is not None and not (0.0 < perplexity and 3.0 * perplexity < N):
        raise ValueError("%s: perplexity %g with %d points; it must lie in (0, N/3) = (0, %g)" % (what, perplexity, N, N / 3.0))


def _tsne_scratch(lib, N, D, device):
    return torch.empty(lib.t2v_tsne_scratch_bytes(N, D), device=device, dtype=torch.uint8)


def tsne_learning_rate(N):
    """scikit-learn's learning_rate='auto': max(N / early_exaggeration / 4, 50)"""
    return max(N / 12.0 / 4.0, 50.0)


def tsne_affinities(x, perplexity=30.0):
    """The joint probabilities of exact t-SNE (csrc/tsne.hip k_tsne_cond, k_tsne_sym): x (N, D) float32 CUDA tensor ->
    dense (N, N) float32 P, P_ij = (p_j|i + p_i|j) / (2N), each row's Gaussian fitted to `perplexity` by a 100-step binary
    search (entropy tolerance 1e-5).  P is symmetric to the bit and its diagonal is 0.  Only x[:N] is read."""
    lib = _require_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("tsne_affinities: x must be a float32 (N, D) tensor")
    N, D = x.shape
    perplexity = float(perplexity)
    _tsne_check("tsne_affinities", N, D, perplexity)
    x = _f32c(x)
    P = torch.empty(N, N, device=x.device, dtype=torch.float32)
    _check(lib.t2v_tsne_affinities(_p(x), N, D, perplexity, _p(P), None, _stream()), 't2v_tsne_affinities')
    return P


def tsne_gradient(P, Y, exaggeration=1.0):
    """One all-pairs pass at the map Y (N, 2) with the symmetric P (N, N) of tsne_affinities (k_tsne_pairs, k_tsne_finish):
    returns (grad (N, 2), kl ()), the gradient of the KL divergence of exaggeration * P from the Student-t Q of Y, and that
    divergence."""
    lib = _require_gpu(P, Y)
    if P.dim() != 2 or P.size(0) != P.size(1) or P.dtype != torch.float32:
        raise ValueError("tsne_gradient: P must be a float32 (N, N) tensor, got %s" % (tuple(P.shape),))
    N = P.size(0)
    if tuple(Y.shape) != (N, 2) or Y.dtype != torch.float32:
        raise ValueError("tsne_gradient: Y must be a float32 (%d, 2) tensor, got %s" % (N, tuple(Y.shape)))
    _tsne_check("tsne_gradient", N)
    if not float(exaggeration) > 0.0:
        raise ValueError("tsne_gradient: exaggeration %g must be positive" % exaggeration)
    P, Y = _f32c(P), _f32c(Y)
    grad = torch.empty(N, 2, device=P.device, dtype=torch.float32)
    kl = torch.empty((), device=P.device, dtype=torch.float32)
    scratch = _tsne_scratch(lib, N, 2, P.device)
    _check(lib.t2v_tsne_gradient(_p(P), _p(Y), N, float(exaggeration), _p(grad), _p(kl), _p(scratch), _stream()),
           't2v_tsne_gradient')
    return grad, kl


def tsne_init(N, seed=0):
    """scikit-learn's init='random': 1e-4 * standard_normal((N, 2)) of a numpy RandomState(seed), as float32"""
    import numpy as np
    return torch.from_numpy((1e-4 * np.random.RandomState(seed).standard_normal(size=(N, 2))).astype(np.float32))


def tsne(x, perplexity=30.0, n_iter=1000, seed=0, init=None, return_trace=False):
    """Exact t-SNE of x (N, D) float32 CUDA tensor to a (N, 2) float32 map on x's device (csrc/tsne.hip): affinities once,
    then n_iter iterations of scikit-learn's gradient descent (250 at exaggeration 12 and momentum 0.5, then 1 and 0.8;
    learning rate max(N / 48, 50); gains) queued on the current stream; no early stop, no host synchronisation.
    init: a (N, 2) start, else tsne_init(N, seed).  return_trace: also the KL divergence after 50, 100, ..., n_iter
    iterations (a float32 device tensor; its last entry is the final map's).  Equal inputs give equal bits."""
    lib = _require_gpu(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("tsne: x must be a float32 (N, D) tensor")
    N, D = x.shape
    perplexity, n_iter = float(perplexity), int(n_iter)
    _tsne_check("tsne", N, D, perplexity)
    if n_iter < 1:
        raise ValueError("tsne: n_iter %d must be >= 1" % n_iter)
    if init is None:
        Y = tsne_init(N, seed).to(x.device)
    else:
        init = torch.as_tensor(init)
        if tuple(init.shape) != (N, 2):
            raise ValueError("tsne: init must be (%d, 2), got %s" % (N, tuple(init.shape)))
        Y = init.to(device=x.device, dtype=torch.float32).contiguous().clone()
    P = tsne_affinities(x, perplexity)
    trace = torch.empty((n_iter + TSNE_KL_EVERY - 1) // TSNE_KL_EVERY, device=x.device, dtype=torch.float32)
    scratch = _tsne_scratch(lib, N, D, x.device)
    _check(lib.t2v_tsne_run(_p(P), _p(Y), N, n_iter, tsne_learning_rate(N), _p(trace), _p(scratch), _stream()), 't2v_tsne_run')
    return (Y, trace) if return_trace else Y


LATENT_MAX_POINTS = _ABI.define('T2V_LATENT_MAX_POINTS')
LATENT_MAX_DIM = 64
LATENT_MAX_CLASSES = _ABI.define('T2V_LATENT_MAX_CLASSES')
LATENT_MAX_K = _ABI.define('T2V_LATENT_MAX_K')
LATENT_TILE = _ABI.define('T2V_LATENT_TILE')      # slice_rows is a multiple of it

LatentNeighbours = collections.namedtuple('LatentNeighbours', 'idx dist class_sum class_cnt rank')


def _latent_check(what, N, M, D, C, k, excluding):
    for name, v in (('refs', N), ('queries', M)):
        if v < 2 or v > LATENT_MAX_POINTS:
            raise ValueError("%s: %s has %d rows; 2..%d are supported" % (what, name, v, LATENT_MAX_POINTS))
    if D < 2 or D > LATENT_MAX_DIM:
        raise ValueError("%s: refs has %d dimensions; 2..%d are supported" % (what, D, LATENT_MAX_DIM))
    if isinstance(C, bool) or int(C) != C or C < 1 or C > LATENT_MAX_CLASSES:
        raise ValueError("%s: n_classes %r; 1..%d are supported" % (what, C, LATENT_MAX_CLASSES))
    if isinstance(k, bool) or int(k) != k or k < 1 or k > LATENT_MAX_K:
        raise ValueError("%s: k %r; 1..%d are supported" % (what, k, LATENT_MAX_K))
    most = N - 1 if excluding else N
    if k > most:
        raise ValueError("%s: k %d, but a query has only %d references to choose from (%d refs%s)"
                         % (what, k, most, N, ", one excluded" if excluding else ""))


def _latent_indices(what, name, v, count, lo, hi, device):
    """an index argument of latent_neighbours as a device int32 vector: `count` integers in lo..hi, else a ValueError that names
    the first offending position"""
    n = torch.as_tensor(v).reshape(-1).cpu()
    if n.dtype.is_floating_point or n.dtype == torch.bool or n.numel() != count:
        raise ValueError("%s: %s must be %d integers, got %s %s" % (what, name, count, n.dtype, tuple(torch.as_tensor(v).shape)))
    n = n.to(torch.int64)
    bad = ((n < lo) | (n > hi)).nonzero()
    if len(bad):
        at = int(bad[0])
        raise ValueError("%s: %s[%d] = %d lies outside %d..%d" % (what, name, at, int(n[at]), lo, hi))
    return n.to(torch.int32).to(device)


def latent_neighbours(refs, labels, queries=None, k=5, n_classes=4, exclude=None, target=None, slice_rows=0):
    """Neighbours and class distances in a labelled latent space (csrc/latent.hip k_latent_pairs + k_latent_merge): refs (N, D)
    float32 CUDA tensor, labels N integers in 0..n_classes-1, queries (M, D) or None for the refs themselves.  exclude: M
    reference indices (-1: none) that the query skips; with queries None and exclude None each row skips itself (leave one
    out).  target: M reference indices (-1: none) whose rank is wanted.  Returns LatentNeighbours of device tensors:
      idx (M, k) int32, dist (M, k) float32: the k nearest non-excluded references by (squared distance, index), ties to the
        lower index, and their Euclidean distances;   class_sum (M, n_classes) float32, class_cnt (M, n_classes) int32: sum
        of distances to, and count of, the non-excluded references of each class;   rank (M,) int32: how many references sort
        strictly before the target (exclusion does not apply), -1 without one.
    Distances come from the differences, so integer inputs give exact ties.  Equal inputs give equal bits; slice_rows (0, or a
    multiple of LATENT_TILE: how many references one workgroup visits) changes the launch and no bit of the result.
    Labels and indices are checked here, on the host (one copy each): a ValueError names the first offending position."""
    what = "latent_neighbours"
    for name, v in (('refs', refs), ('queries', queries)):
        if v is None and name == 'queries':
            continue
        if not torch.is_tensor(v) or v.dim() != 2 or v.dtype != torch.float32:
            raise ValueError("%s: %s must be a float32 (rows, D) tensor, got %s %s"
                             % (what, name, getattr(v, 'dtype', type(v)), tuple(getattr(v, 'shape', ()))))
    lib = _require_gpu(refs, queries)
    N, D = refs.shape
    M = N if queries is None else queries.size(0)
    if queries is not None and queries.size(1) != D:
        raise ValueError("%s: queries have %d dimensions, refs %d" % (what, queries.size(1), D))
    excluding = exclude is not None or queries is None
    _latent_check(what, N, M, D, n_classes, k, excluding)
    if isinstance(slice_rows, bool) or int(slice_rows) != slice_rows or slice_rows < 0 or slice_rows % LATENT_TILE:
        raise ValueError("%s: slice_rows %r must be 0 or a positive multiple of %d" % (what, slice_rows, LATENT_TILE))
    dev = refs.device
    lab = _latent_indices(what, 'labels', labels, N, 0, n_classes - 1, dev)
    ex = None if exclude is None else _latent_indices(what, 'exclude', exclude, M, -1, N - 1, dev)
    tg = None if target is None else _latent_indices(what, 'target', target, M, -1, N - 1, dev)
    refs = _f32c(refs)
    queries = None if queries is None else _f32c(queries)
    if not bool(torch.isfinite(refs).all()) or (queries is not None and not bool(torch.isfinite(queries).all())):
        raise ValueError("%s: refs and queries must be finite" % what)
    k, C_, slice_rows = int(k), int(n_classes), int(slice_rows)
    idx = torch.empty(M, k, device=dev, dtype=torch.int32)
    dist = torch.empty(M, k, device=dev, dtype=torch.float32)
    class_sum = torch.empty(M, C_, device=dev, dtype=torch.float32)
    class_cnt = torch.empty(M, C_, device=dev, dtype=torch.int32)
    rank = torch.empty(M, device=dev, dtype=torch.int32)
    scratch = torch.empty(lib.t2v_latent_scratch_bytes(N, M, C_, k, slice_rows), device=dev, dtype=torch.uint8)
    _check(lib.t2v_latent_neighbours(_p(refs), _p(lab), N, D, C_, _p(queries), M, _p(ex), _p(tg), k, slice_rows, _p(idx),
                                     _p(dist), _p(class_sum), _p(class_cnt), _p(rank), _p(scratch), _stream()),
           't2v_latent_neighbours')
    return LatentNeighbours(idx, dist, class_sum, class_cnt, rank)


def check_attention_window(window):
    """None, or (back, ahead) as a tuple of two Python ints >= 0; anything else raises ValueError"""
    if window is None:
        return None
    try:
        if isinstance(window, (str, bytes)) or any(isinstance(x, bool) for x in window):
            raise TypeError
        vals = tuple(operator.index(x) for x in window)
    except TypeError:
        vals = ()
    if len(vals) != 2 or min(vals) < 0 or max(vals) > 2 ** 31 - 1:
        raise ValueError("attention_window must be None or (back, ahead), two integers >= 0, got %r" % (window,))
    return vals


PLAN_MAX_SYMBOLS = _ABI.define('T2V_PLAN_MAX_SYMBOLS')      # the frame ends of a row sit in LDS
PLAN_MAX_FRAMES_PER_SYMBOL = 2 ** 20

DurationPlan = collections.namedtuple('DurationPlan', 'plan n_plan')
DurationPlan.__doc__ = """What duration_plan() returns.  plan (B, T_max) int32: the symbol of every frame, the last one held
behind n_plan[b] (0 for an empty plan); n_plan (B,) int32: min(total frames, T_max)."""


def duration_plan(dur, n_ids, T_max, rate=None):
    """Length regulator (csrc/plan.hip k_duration_plan): symbol durations -> the frame-by-frame plan of a planned decode.
    dur: (B, S) float32 CUDA tensor, frames per symbol (fractions allowed); n_ids: B symbol counts in 0..S (a list, a CPU or a
    device tensor); rate: None, a number, or a (B, S) float32 tensor of factors multiplied in; T_max: the plan's width.
    In integers (include/t2vae.h): q_j = rint(dur_j rate_j 65536) in fp64, C = cumsum(q), E_j = (C_j + 32768) >> 16; symbol j
    owns the frames E_{j-1} <= t < E_j (none: skipped); n_plan = min(E_last, T_max).  A row gives the same plan alone and in
    any batch.  Returns a DurationPlan.  A row with a negative or non-finite dur * rate, or one above 2^20 frames per symbol,
    is a ValueError naming the row (this reads n_plan back: one synchronisation)."""
    lib = load_library()
    if not torch.is_tensor(dur) or dur.dim() != 2 or dur.dtype != torch.float32 or dur.size(0) < 1 or dur.size(1) < 1:
        raise ValueError("duration_plan: dur must be a non-empty float32 (B, S) tensor, got %s %s"
                         % (getattr(dur, 'dtype', type(dur)), tuple(getattr(dur, 'shape', ()))))
    if not dur.is_cuda:
        raise T2VHipError("duration_plan: dur %s lives on %s; this path has no CPU fallback" % (tuple(dur.shape), dur.device))
    B, S = dur.shape
    if S > PLAN_MAX_SYMBOLS:
        raise ValueError("duration_plan: %d symbols per row; at most %d are supported" % (S, PLAN_MAX_SYMBOLS))
    if isinstance(T_max, bool) or int(T_max) != T_max or not 1 <= T_max <= 2 ** 31 - 1:
        raise ValueError("duration_plan: T_max %r must be an integer >= 1" % (T_max,))
    T_max = int(T_max)
    dev = dur.device
    dur = dur.contiguous()
    L = _checked_lengths(n_ids, B, 0, S, "duration_plan: n_ids must be %d integer symbol counts" % B,
                         "duration_plan: every n_ids must be in 0..%d (symbols stored per row)" % S).to(dev)
    rsb = rsj = 0
    if rate is None:
        r = None
    elif torch.is_tensor(rate) and rate.dim() > 0:
        if rate.shape != dur.shape or rate.dtype != torch.float32 or rate.device != dev:
            raise ValueError("duration_plan: a rate tensor must be float32 %s on %s, got %s %s on %s"
                             % (tuple(dur.shape), dev, rate.dtype, tuple(rate.shape), rate.device))
        r, rsb, rsj = rate.contiguous(), S, 1
    else:
        r = torch.full((1,), float(rate), dtype=torch.float32).to(dev)       # a scalar on the device: both strides 0
    plan = torch.empty(B, T_max, device=dev, dtype=torch.int32)
    n_plan = torch.empty(B, device=dev, dtype=torch.int32)
    _check(lib.t2v_duration_plan(_p(dur), S, _p(L), _p(r), rsb, rsj, B, S, T_max, _p(plan), T_max, _p(n_plan), _stream()),
           't2v_duration_plan')
    bad = [b for b, n in enumerate(n_plan.tolist()) if n < 0]
    if bad:
        raise ValueError("duration_plan: row %s: every dur * rate must be finite and in 0..%d frames"
                         % (', '.join(str(b) for b in bad), PLAN_MAX_FRAMES_PER_SYMBOL))
    return DurationPlan(plan, n_plan)


def check_plan(plan, n_plan, B, max_steps, device, window):
    """The plan of a planned decode (include/t2vae.h t2v_decoder_infer_steps_plan), checked on the host: plan an int32 (B, N)
    tensor on `device` with last stride 1 and N <= max_steps columns, n_plan B int32 counts on `device` in 1..N, `window` a
    (back, ahead).  Returns (plan, n_plan as a host list); anything else raises ValueError.  Reads n_plan back (one
    synchronisation, at session set-up)."""
    if window is None:
        raise ValueError("a plan needs a window (back, ahead) around its symbols; (0, 0) is the one-hot form")
    for name, t in (('plan', plan), ('n_plan', n_plan)):
        if not torch.is_tensor(t) or t.dtype != torch.int32:
            raise ValueError("%s must be an int32 tensor, got %s" % (name, getattr(t, 'dtype', type(t))))
        if t.device != torch.device(device):
            raise ValueError("%s lives on %s; the decode runs on %s" % (name, t.device, device))
    if plan.dim() != 2 or plan.size(0) != B or plan.size(1) < 1 or (plan.size(1) > 1 and plan.stride(1) != 1) or \
            (B > 1 and plan.stride(0) < plan.size(1)):
        raise ValueError("plan must be (%d, N >= 1) with rows of stride 1, got %s strides %s" % (B, tuple(plan.shape), plan.stride()))
    if tuple(n_plan.shape) != (B,):
        raise ValueError("n_plan must hold %d frame counts, got %s" % (B, tuple(n_plan.shape)))
    n = n_plan.tolist()
    if min(n) < 1 or max(n) > plan.size(1):
        raise ValueError("every n_plan must be in 1..%d (the plan's columns), got %s" % (plan.size(1), n))
    if max(n) > max_steps:
        raise ValueError("a plan of %d frames is longer than the %d decoder steps of this session" % (max(n), max_steps))
    return plan, n


class InferenceSession(object):
    """Arena + packed weights of one free-running decode (Decoder.inference / the per-step
    initialize_decoder_states → prenet → decode call sequence of synthesizer.py:135-154)."""
    INT_MAX = 2 ** 31 - 1

    def __init__(self, memory, pm, lengths, w_ih_att, w_hh_att, b_att, w_ih_dec, w_hh_dec, b_dec, wq, loc_conv,
                 loc_dense, v, prenet_w0, prenet_w1, proj_w, proj_b, gate_w, gate_b, max_steps, item_seeds=None,
                 attention_window=None, plan=None, n_plan=None, n_plan_host=None):
        if 'T2V_HOST_THREADS' in os.environ:        # (an inference session no longer throttles the host application)
            limit_host_threads()
        lib = _require_gpu(memory, pm, w_ih_att)
        B, T_in, _ = memory.shape
        if B > 8:
            raise T2VHipError("one decode session takes B <= 8 utterances (Decoder.inference runs larger batches 8 at a time)")
        dev = memory.device
        f32 = dict(device=dev, dtype=torch.float32)
        self.B, self.T_in, self.max_steps = B, T_in, int(max_steps)
        T = self.max_steps
        self.memory, self.pm, self.lengths = _f32c(memory.detach()), _f32c(pm.detach()), lengths
        # the persistent one-launch loop reads the nn.LSTMCell tensors themselves (weights stay in registers); the 71 MB pack
        # of the launch-per-stage loop is built by the first run() that needs it (round 4: it cost every utterance ~0.1 ms)
        self.packF_att = self.packF_dec = self.W = None
        self.raw = tuple(_f32c(t.detach()) for t in (w_ih_att, w_hh_att, w_ih_dec, w_hh_dec))
        self.wq = _f32c(wq.detach())
        self.b_att, self.b_dec = _f32c(b_att.detach()), _f32c(b_dec.detach())
        self.wqT = wq.detach().t().contiguous()
        self.wcomb = fuse_location_weights(_f32c(loc_conv.detach()), _f32c(loc_dense.detach()))
        self.v = _f32c(v.detach()).view(-1)
        self.w1 = _f32c(prenet_w1.detach())
        # Prenet layer 0 (bias-free, linear in the mel frame) folded into the projection: rows 81.. = W0·P, W0·b
        w0 = _f32c(prenet_w0.detach())
        pw, pb = _f32c(proj_w.detach()), _f32c(proj_b.detach())
        w0p = gemm(w0, pw.t())                                                   # (256,1536) = W0 (256,80) · P (80,1536)
        b0p = gemm(w0, pb.view(1, -1)).view(-1)                                  # (256) = W0 · b
        self.proj_w = torch.cat((pw, gate_w.detach(), w0p), 0).contiguous()      # (337,1536)
        self.proj_b = torch.cat((pb, gate_b.detach(), b0p), 0).contiguous()
        # the persistent launch keeps the recurrent state on chip: it needs PRE[0] and writes MEL / GATE / AL / stop.  The state
        # arenas of the launch-per-stage loop (XS, CA, CD, QP, ACUM: 20 MB, five clears) are made by the first run() (round 4)
        self.XS = self.CA = self.CD = self.QP = self.ACUM = self.S = None
        self.AL = torch.empty(T + 1, B, T_in, **f32); self.AL[0].zero_()
        self.PRE = torch.empty(T + 1, B, PRE, **f32)
        self.MEL = torch.empty(T, B, 80, **f32)
        self.GATE = torch.empty(T, B, **f32)
        self.stop = torch.full((1,), self.INT_MAX, device=dev, dtype=torch.int32)
        self.t = 0
        # item_seeds (B ints): per-item Prenet dropout seeds — item b's masks are those of a B = 1 decode with seed
        # item_seeds[b] — and per-item stop frames (stop_item[b]: first frame on which item b's gate fired, INT_MAX if none)
        self.item_seeds = self.stop_item = self._items = None
        if item_seeds is not None:
            if len(item_seeds) != B:
                raise T2VHipError("item_seeds: %d seeds for %d utterances" % (len(item_seeds), B))
            seeds = [int(x) & 0xFFFFFFFFFFFFFFFF for x in item_seeds]
            seeds = [x - (1 << 64) if x >= (1 << 63) else x for x in seeds]            # the bits as a signed int64
            self.item_seeds = torch.tensor(seeds, dtype=torch.int64).to(dev)
            self.stop_item = torch.full((B,), self.INT_MAX, device=dev, dtype=torch.int32)
            self._items = _DecItems(_p(self.stop_item), _p(self.item_seeds))
        # attention_window (back, ahead): every frame's energies are masked to [p - back, p + ahead] around the position p of
        # the previous frame's largest weight (include/t2vae.h t2v_dec_window); both decode loops, every run of this session
        self.attention_window = check_attention_window(attention_window)
        self._window = None if self.attention_window is None else _DecWindow(*self.attention_window)
        # plan (B, N) int32, n_plan (B) int32 on the device: the window's centre of frame t is plan[b, min(t, n_plan[b] - 1)]
        # instead of the previous frame's largest weight (include/t2vae.h t2v_decoder_infer_steps_plan); both decode loops
        # (n_plan_host: the counts as a check_plan of the caller's has read them back already; no second synchronisation)
        self.plan = self.n_plan = self.n_plan_host = None
        if plan is not None or n_plan is not None:
            if n_plan_host is None:
                plan, n_plan_host = check_plan(plan, n_plan, B, self.max_steps, dev, self.attention_window)
            self.plan, self.n_plan, self.n_plan_host = plan, n_plan, [int(x) for x in n_plan_host]

    def _constrained(self, name, args):
        """the entry point and arguments of a run under the session's constraints: *_plan (items or NULL, the window, the
        plan), *_window (items or NULL, the window), *_items, or the plain entry"""
        items = None if self._items is None else C.byref(self._items)
        if self.plan is not None:
            stride = self.plan.stride(0) if self.B > 1 else self.plan.size(1)
            return name + '_plan', args + [items, C.byref(self._window), _p(self.plan), stride, _p(self.n_plan)]
        if self._window is not None:
            return name + '_window', args + [items, C.byref(self._window)]
        if self._items is not None:
            return name + '_items', args + [items]
        return name, args

    def _stage_arena(self):
        if self.S is not None:
            return
        lib = load_library()
        B, T_in, T = self.B, self.T_in, self.max_steps
        f32 = dict(device=self.memory.device, dtype=torch.float32)
        self.XS = torch.empty(T + 2, B, XW, **f32); self.XS[0:2].zero_()
        self.CA = torch.empty(T + 1, B, H, **f32); self.CA[0].zero_()
        self.CD = torch.empty(T + 1, B, H, **f32); self.CD[0].zero_()
        self.QP = torch.empty(lib.t2v_decoder_qp_floats(B, T_in), **f32)
        self.ACUM = torch.empty(T + 1, B, T_in, **f32); self.ACUM[0].zero_()
        self.S = _DecInferBufs(_p(self.memory), _p(self.pm), _p(self.lengths), _p(self.XS), _p(self.CA), _p(self.CD),
                               _p(self.QP), _p(self.AL), _p(self.ACUM), _p(self.PRE), _p(self.MEL), _p(self.GATE),
                               _p(self.stop), _p(self.w1), _p(self.proj_w), _p(self.proj_b))

    def persistent_supported(self):
        return bool(load_library().t2v_decoder_persist_supported(self.B, self.T_in))

    def run_persistent(self, gate_threshold, p_prenet, seed):
        """frames 0..max_steps-1 (or up to the frame the gate fires) as ONE persistent launch (csrc/decoder_persist.hip);
        PRE[0] must hold Prenet(go frame).  Outputs: MEL, GATE, AL, stop."""
        lib = load_library()
        dev = self.memory.device
        if not hasattr(self, '_gran'):
            self._gran = torch.empty(lib.t2v_decoder_persist_scratch_floats(self.B, self.max_steps), device=dev, dtype=torch.float32)
            self._perr = torch.zeros(1, device=dev, dtype=torch.int32)
        W = _DecPersistWeights(_p(self.raw[0]), _p(self.raw[1]), _p(self.raw[2]), _p(self.raw[3]), _p(self.b_att), _p(self.b_dec),
                               _p(self.wq), _p(self.wcomb), _p(self.v), _p(self.proj_w), _p(self.proj_b), _p(self.w1))
        Bf = _DecPersistBufs(_p(self.memory), _p(self.pm), _p(self.lengths), _p(self.PRE[0]), _p(self.MEL), _p(self.GATE),
                             _p(self.AL), _p(self.stop), _p(self._gran), _p(self._perr))
        name, args = 't2v_decoder_infer_persistent', [C.byref(W), C.byref(Bf), self.B, self.T_in, self.max_steps,
                                                      float(gate_threshold), float(p_prenet), int(seed)]
        name, args = self._constrained(name, args)
        _check(getattr(lib, name)(*args, _stream()), name)

    def persistent_timed_out(self):
        """True when a bounded spin of the last run_persistent() gave up (the 256 workgroups were not co-resident);
        synchronises — Decoder.inference reads the stop frame at the same point anyway"""
        return bool(self._perr.item())

    def reset_for_rerun(self):
        """after a failed persistent run: the launch-per-stage loop starts again from the zero state (rows 0 of the state
        arenas are still zero — the persistent kernel keeps its state on chip — and PRE[0] still holds Prenet(go frame))"""
        self.stop.fill_(self.INT_MAX)
        if self.stop_item is not None:
            self.stop_item.fill_(self.INT_MAX)
        self._perr.zero_()

    def run(self, t0, t1, gate_threshold, p_prenet, external_prenet, seed):
        self._stage_arena()
        if self.W is None:
            self.packF_att, self.packF_dec, _, _ = pack_decoder_weights(self.raw[0], self.raw[1], self.raw[2], self.raw[3], KATT_INF,
                                                                        False)
            self.W = _DecWeights(_p(self.packF_att), _p(self.packF_dec), None, None, _p(self.b_att), _p(self.b_dec),
                                 _p(self.wqT), _p(self.wcomb), _p(self.v))
        name, args = 't2v_decoder_infer_steps', [C.byref(self.W), C.byref(self.S), self.B, self.T_in, int(t0), int(t1),
                                                 float(gate_threshold), float(p_prenet), int(bool(external_prenet)), int(seed)]
        name, args = self._constrained(name, args)
        _check(getattr(load_library(), name)(*args, _stream()), name)


def limit_host_threads(n=None):
    """Cap torch's intra-op (OpenMP) host threads for the training process (default 4, env T2V_HOST_THREADS; 0 = leave).
    Every step touches a few host tensors (the 768 KB mel of the collated batch is copied into the pinned staging buffer
    with a parallel copy); on a 256-thread host torch starts 128 workers for that, and they spin after the region.  The GPU
    boxes run containers with a CPU quota (cgroup cpu.max = 16 CPUs per 100 ms): the spinning workers exhaust it and the
    WHOLE process — the thread that feeds the GPU included — is frozen for the rest of each period.  Measured: eager steps
    13.7, 13.7, 71 ms, ... (every ~100 ms an ~60 ms freeze; 33–39 ms per step on average) against a steady 13.7 ms with 4
    threads; the replayed-graph step 14.07 -> 13.43 ms.  Data-loader workers are separate processes and unaffected."""
    prev = torch.get_num_threads()
    if n is None:
        n = int(os.environ.get('T2V_HOST_THREADS', '2' if int(os.environ.get('WORLD_SIZE', '1')) > 1 else '4'))
    if n > 0 and prev > n:
        torch.set_num_threads(n)
    return prev         # (the training engine restores it in close(): the cap belongs to the training loop, not to the host app)


ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2


# ---- data-gradient operands of the k=5 convolutions, flipped once per step (Tacotron2._forward issues ONE launch for the
# eight layers on the deferred-work stream during the forward pass) instead of one flip launch in front of every dX conv
_PREFLIP = {}


def preflip_conv_weights(weights):
    """weights: fp32 (Cout, Cin, KS) conv weights with one common KS.  Fills _PREFLIP[data_ptr] = flipped copy; the
    ConvBNAct1d backward of this step picks it up (and falls back to its own flip launch when there is none)."""
    lib = load_library()
    _PREFLIP.clear()
    ws = [w.detach() for w in weights if w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()]
    if not ws or _BF16:
        return
    n = len(ws)
    KS = ws[0].shape[2]
    if n > 16 or any(w.shape[2] != KS for w in ws):
        return
    total = sum(w.numel() for w in ws)
    flat = torch.empty(total, device=ws[0].device, dtype=torch.float32)
    outs, o = [], 0
    for w in ws:
        outs.append(flat[o:o + w.numel()].view(w.shape[1], w.shape[0], KS))
        o += w.numel()
    PA, IA = C.c_void_p * n, C.c_int * n
    _check(lib.t2v_conv1d_flip_weights(PA(*[w.data_ptr() for w in ws]), PA(*[t.data_ptr() for t in outs]),
                                       IA(*[w.shape[0] for w in ws]), IA(*[w.shape[1] for w in ws]), int(KS), n, _stream()),
           't2v_conv1d_flip_weights')
    ev = torch.cuda.Event()
    ev.record()             # consumers on another stream wait for THIS point, not for whatever that stream is doing by then
    st = torch.cuda.current_stream()
    for w, t in zip(ws, outs):
        _PREFLIP[w.data_ptr()] = (t, st, ev)


def _conv_bf16(Cin, Cout, KS):
    """bf16_run: does the Conv1d Cin -> Cout run on the bf16 entry points?  Only the wide layers (the three 512->512 Postnet
    convs, the encoder bank); the 80-channel first and last Postnet layers are cheap and stay fp32 (the output layer in
    particular)"""
    return _BF16 and KS == 5 and Cin % 16 == 0 and Cin >= 128 and Cout >= 128


def _conv1d_fwd(lib, w, x, bias, y, want_stats):
    """y = Conv1d(x) + bias by the fp32 or the bf16_run entry point.  Returns (part, nblk): the BatchNorm partials the
    launch wrote (None unless want_stats) and their block count, which the library answers from the route the launch takes"""
    B, Cin, T = x.shape
    Cout, _, KS = w.shape
    bf16 = _conv_bf16(Cin, Cout, KS)
    nblk = (lib.t2v_conv1d_stat_blocks_bf16 if bf16 else lib.t2v_conv1d_stat_blocks)(B, T, Cin, Cout, KS)
    part = torch.empty(nblk, Cout, 2, device=x.device, dtype=torch.float32) if want_stats else None
    if bf16:
        wp = torch.empty(w.numel(), device=x.device, dtype=torch.bfloat16)
        _check(lib.t2v_conv1d_fwd_bf16(_p(w), _p(x), _p(bias), _p(y), _p(part), _p(wp), B, Cin, T, Cout, KS, _stream()),
               't2v_conv1d_fwd_bf16')
    else:
        _check(lib.t2v_conv1d_fwd(_p(w), _p(x), _p(bias), _p(y), _p(part), B, Cin, T, Cout, KS, _stream()), 't2v_conv1d_fwd')
    return part, nblk


class ConvBNAct1d(torch.autograd.Function):
    """dropout(act(BatchNorm1d(Conv1d(x)))) — one block of the encoder conv bank / Postnet
    (reference model.py:143-148, 175-177) on the HIP implicit-GEMM conv + per-channel BN kernels.
    `x` is saved by reference: the in-place output masking of reference model.py:515 therefore reaches
    the first Postnet block's weight gradient exactly like it does in the reference (Appendix B-5)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, training, act, p_drop, seed,
                rng_stream, rng_t):
        lib = _require_gpu(x, weight)
        x = x if x.is_contiguous() else x.contiguous()
        B, Cin, T = x.shape
        Cout, _, KS = weight.shape
        dev = x.device
        f32 = dict(device=dev, dtype=torch.float32)
        y = torch.empty(B, Cout, T, **f32)
        w = weight.contiguous()
        part, nblk = _conv1d_fwd(lib, w, x, bias, y, training)
        mean = torch.empty(Cout, **f32) if training else None
        rstd = torch.empty(Cout, **f32) if training else None
        out = torch.empty(B, Cout, T, **f32)
        _check(lib.t2v_bn_act_fwd(_p(y), _p(part), nblk, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                                  _p(mean), _p(rstd), _p(out), B, Cout, T, int(act), int(bool(training)),
                                  float(p_drop if training else 0.0), 0.1, 1e-5, int(seed), int(rng_stream),
                                  int(rng_t), _stream()), 't2v_bn_act_fwd')
        ctx.cfg = (B, Cin, T, Cout, KS, int(act), float(p_drop if training else 0.0), int(seed), int(rng_stream),
                   int(rng_t), bool(training))
        ctx.keep = (x, w, y, mean, rstd, gamma, beta, running_mean, running_var)
        ctx.small = (gamma, beta, bias)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = load_library()
        B, Cin, T, Cout, KS, act, p, seed, rs, rt, training = ctx.cfg
        x, w, y, mean, rstd, gamma, beta, running_mean, running_var = ctx.keep
        f32 = dict(device=x.device, dtype=torch.float32)
        bn_bwd = lib.t2v_bn_act_bwd
        if not training:   # eval-mode BN backward (model.eval() with gradients, e.g. fine-tuning with frozen statistics)
            mean = running_mean
            rstd = torch.rsqrt(running_var + 1e-5)
            bn_bwd = lib.t2v_bn_act_bwd_eval
        dout = dout.contiguous()
        dy = torch.empty(B, Cout, T, **f32)
        # d(bias) of a conv feeding a training-mode BatchNorm is identically zero (dy has zero channel mean): the BN
        # kernel writes those zeros along with dgamma / dbeta (eval mode: the real bias gradient)
        dgamma, dbeta, dbias = _small_grads(ctx.small, Cout, f32)
        _check(bn_bwd(_p(y), _p(dout), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dy), _p(dgamma),
                      _p(dbeta), _p(dbias), B, Cout, T, act, p, seed, rs, rt, _stream()), 't2v_bn_act_bwd')
        need_dx = ctx.needs_input_grad[0]
        dx = torch.empty(B, Cin, T, **f32) if need_dx else None
        fork = mark()       # the weight gradient below depends on dy only: it forks from HERE, not from behind the dX conv
        # the data gradient (what the next layer down waits for) on the current stream ...
        if need_dx and _conv_bf16(Cin, Cout, KS) and Cout % 16 == 0:
            wp = torch.empty(w.numel(), device=x.device, dtype=torch.bfloat16)
            _check(lib.t2v_conv1d_bwd_bf16(_p(w), _p(x), _p(dy), _p(dx), None, _p(wp), None, B, Cin, T, Cout, KS,
                                           _stream()), 't2v_conv1d_bwd_bf16')
        elif need_dx:
            pre = _PREFLIP.get(w.data_ptr())
            if pre is not None and pre[0].numel() == w.numel():
                wt, st, ev = pre
                if st != torch.cuda.current_stream():
                    torch.cuda.current_stream().wait_event(ev)          # flipped on the deferred-work stream, long ago
                _check(lib.t2v_conv1d_bwd(None, _p(x), _p(dy), _p(dx), None, _p(wt), None, B, Cin, T, Cout, KS,
                                          _stream()), 't2v_conv1d_bwd')
            else:
                wt = torch.empty_like(w)
                _check(lib.t2v_conv1d_bwd(_p(w), _p(x), _p(dy), _p(dx), None, _p(wt), None, B, Cin, T, Cout, KS,
                                          _stream()), 't2v_conv1d_bwd')
        # ... the weight gradient (nobody waits for it before the optimiser) on the engine's deferred-work stream
        with side('w', keep=(x, dy), after=fork):
            dw = grad_slot(w)
            dw = torch.empty_like(w) if dw is None else dw
            nscr = lib.t2v_conv1d_dw_scratch_floats(B, Cin, T, Cout, KS)
            scr = torch.empty(nscr, **f32) if nscr else None
            if _BF16 and KS == 5 and Cin % 16 == 0 and os.environ.get('T2V_CONV_DW_BF16', '1') != '0':
                # (round 5) bf16_run: the weight gradient on bf16 MFMA too (dY, X rounded while staged; fp32 accumulation)
                _check(lib.t2v_conv1d_bwd_bf16(None, _p(x), _p(dy), None, _p(dw), None, _p(scr), B, Cin, T, Cout, KS,
                                               _stream()), 't2v_conv1d_bwd_bf16')
            else:
                _check(lib.t2v_conv1d_bwd(None, _p(x), _p(dy), None, _p(dw), None, _p(scr), B, Cin, T, Cout, KS,
                                          _stream()), 't2v_conv1d_bwd')
        return dx, dw, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None


class SymbolEmbedding(torch.autograd.Function):
    """nn.Embedding lookup of the text encoder (reference model.py:474-482,528).  Returns the (B,T,C) tensor of
    nn.Embedding as a transposed VIEW of a (B,C,T) buffer, so the reference's `.transpose(1, 2)` that follows hands the
    first encoder convolution a contiguous channel-major tensor without a copy."""

    @staticmethod
    def forward(ctx, ids, weight):
        lib = _require_gpu(ids, weight)
        ids = ids.contiguous().long()
        B, T = ids.shape
        n, Cc = weight.shape
        out = torch.empty(B, Cc, T, device=weight.device, dtype=torch.float32)
        _check(lib.t2v_embedding_fwd(_p(ids), _p(_f32c(weight)), _p(out), B, T, Cc, n, _stream()), 't2v_embedding_fwd')
        ctx.save_for_backward(ids)
        ctx.dims = (B, T, Cc, n)
        return out.transpose(1, 2)

    @staticmethod
    def backward(ctx, dy):
        lib = load_library()
        ids, = ctx.saved_tensors
        B, T, Cc, n = ctx.dims
        dy_bct = dy.transpose(1, 2)
        dy_bct = dy_bct if dy_bct.is_contiguous() else dy_bct.contiguous()
        dW = torch.empty(n, Cc, device=dy.device, dtype=torch.float32)
        _check(lib.t2v_embedding_bwd(_p(ids), _p(_f32c(dy_bct)), _p(dW), B, T, Cc, n, _stream()), 't2v_embedding_bwd')
        return None, dW


def mask_outputs(mel, mel_post, gate, lengths_i32, gate_fill=1e3):
    """Tacotron2.parse_output's three in-place fills (reference model.py:513-517) as one launch"""
    lib = _require_gpu(mel, mel_post, gate, lengths_i32)
    assert mel.is_contiguous() and mel_post.is_contiguous() and gate.is_contiguous() and lengths_i32.dtype == torch.int32
    assert mel.dtype == torch.float32 and mel_post.shape == mel.shape and gate.shape == (mel.size(0), mel.size(2))
    B, Cn, T = mel.shape
    _check(lib.t2v_mask_outputs(_p(mel), _p(mel_post), _p(gate), _p(lengths_i32), B, Cn, T, float(gate_fill), _stream()),
           't2v_mask_outputs')


def mask_time(x, lengths_i32):
    """(B,C,T) -> a new tensor equal to x at t < lengths[b] and 0 past it (one launch): the input of a length-masked conv stack"""
    lib = _require_gpu(x, lengths_i32)
    assert x.dim() == 3 and lengths_i32.dtype == torch.int32 and lengths_i32.numel() == x.size(0)
    x = _f32c(x)
    out = torch.empty_like(x)
    B, Cn, T = x.shape
    _check(lib.t2v_mask_time(_p(x), _p(out), _p(lengths_i32), B, Cn, T, _stream()), 't2v_mask_time')
    return out


def conv_bn_act_eval_len(x, weight, bias, gamma, beta, running_mean, running_var, act, lengths_i32):
    """act(BatchNorm1d_eval(Conv1d(x))) over a ragged batch, 0 at every t >= lengths[b]: x must already be 0 there, so each
    item's valid frames are those of the item convolved alone (its zero padding).  No autograd (inference only)."""
    lib = _require_gpu(x, weight, lengths_i32)
    assert lengths_i32.dtype == torch.int32 and lengths_i32.numel() == x.size(0)
    x = _f32c(x)
    B, Cin, T = x.shape
    Cout, _, KS = weight.shape
    y = torch.empty(B, Cout, T, device=x.device, dtype=torch.float32)
    w = _f32c(weight.detach())
    _conv1d_fwd(lib, w, x, bias, y, False)           # the kernel ConvBNAct1d picks
    out = torch.empty_like(y)
    _check(lib.t2v_bn_act_fwd_len(_p(y), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(out), _p(lengths_i32),
                                  B, Cout, T, int(act), 1e-5, _stream()), 't2v_bn_act_fwd_len')
    return out


class Reparam(torch.autograd.Function):
    """z = eps * exp(0.5 logvar) + mu (reference modules.py:74-81) and its gradient, one launch each"""

    @staticmethod
    def forward(ctx, eps, mu, logvar):
        lib = _require_gpu(eps, mu, logvar)
        eps, mu, logvar = _f32c(eps), _f32c(mu), _f32c(logvar)
        z = torch.empty_like(mu)
        _check(lib.t2v_reparam_fwd(_p(eps), _p(mu), _p(logvar), _p(z), mu.numel(), _stream()), 't2v_reparam_fwd')
        ctx.save_for_backward(eps, logvar)
        return z

    @staticmethod
    def backward(ctx, dz):
        eps, logvar = ctx.saved_tensors
        dz = _f32c(dz)
        dlv = torch.empty_like(logvar)
        _check(load_library().t2v_reparam_bwd(_p(dz), _p(eps), _p(logvar), _p(dlv), dz.numel(), _stream()), 't2v_reparam_bwd')
        return None, dz, dlv


class BiLSTM(torch.autograd.Function):
    """Encoder BiLSTM over per-sequence lengths (== pack_padded_sequence → nn.LSTM → pad_packed_sequence,
    reference model.py:183-190).  Input projections / weight gradients are time-batched GEMMs; the
    recurrence (forward and BPTT) runs in the persistent cooperative kernels of csrc/bilstm.hip, 16 sequences per
    call (larger batches run as independent chunks)."""

    _prep = {}      # id(w_hh) -> (whh, bias, bias_r, event): see prepare()

    @staticmethod
    def prepare(w_hh, b_ih, b_hh, w_hh_r, b_ih_r, b_hh_r):
        """the parameter-only operands of forward() (both W_hh stacked, b_ih + b_hh per direction), computed ahead — the
        model issues this on the deferred-work stream at the top of a step, the encoder reaches its BiLSTM 250 us later"""
        with torch.no_grad():
            whh = torch.stack((w_hh, w_hh_r)).contiguous()
            bias, bias_r = b_ih + b_hh, b_ih_r + b_hh_r
        ev = torch.cuda.Event()
        ev.record()
        BiLSTM._prep[id(w_hh)] = (whh, bias, bias_r, ev)

    @staticmethod
    def forward(ctx, x, lengths, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r, save):
        lib = _require_gpu(x, w_ih)
        B, T, _ = x.shape
        f32 = dict(device=x.device, dtype=torch.float32)
        x = _f32c(x)
        prep = BiLSTM._prep.pop(id(w_hh), None)
        if prep is not None:        # stacked recurrent weights / summed biases of this step, made ahead on a side stream
            whh, bias, bias_r, ev = prep
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            for t in (whh, bias, bias_r):
                t.record_stream(cur)
        else:
            whh = torch.stack((w_hh, w_hh_r)).contiguous()
            bias, bias_r = b_ih + b_hh, b_ih_r + b_hh_r
        y = torch.empty(B, T, 512, **f32)       # cleared by t2v_bilstm_fwd's reset launch
        chunks = []
        for b0 in range(0, B, MAX_DEC_B):
            b1 = min(B, b0 + MAX_DEC_B)
            Bc = b1 - b0
            gx = torch.empty(2, Bc, T, 1024, **f32)
            gemm(x[b0:b1].view(Bc * T, -1), w_ih, bias, out=gx[0].view(Bc * T, 1024))
            gemm(x[b0:b1].view(Bc * T, -1), w_ih_r, bias_r, out=gx[1].view(Bc * T, 1024))
            gates = torch.empty(2, Bc, T, 1024, **f32) if save else None
            cells = torch.empty(2, Bc, T, 256, **f32) if save else None
            hx = torch.empty(2 * 2 * 2 * 16 * 256, **f32)              # 8-byte granules
            sync = torch.empty(3, device=x.device, dtype=torch.int32)
            _check(lib.t2v_bilstm_fwd(_p(gx), _p(whh), _p(lengths[b0:b1]), _p(y[b0:b1]), _p(gates), _p(cells), _p(hx),
                                      _p(sync), Bc, T, _stream()), 't2v_bilstm_fwd')
            _err_note('BiLSTM forward', sync[2:3])
            chunks.append((b0, b1, gates, cells, sync))
        # (an alias of y, not y itself: the returned tensor gets this node as its grad_fn — keeping it here would tie the
        # node and its arenas into a reference cycle that only the cyclic GC frees, AccumulateGrad nodes included)
        ctx.keep = (x, lengths, w_ih, w_ih_r, whh, y.detach(), chunks)
        ctx.dims = (B, T)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = load_library()
        x, lengths, w_ih, w_ih_r, whh, y, chunks = ctx.keep
        B, T = ctx.dims
        if chunks[0][2] is None:
            raise T2VHipError("BiLSTM forward ran without saving activations")
        f32 = dict(device=x.device, dtype=torch.float32)
        dy = _f32c(dy)
        dg = torch.empty(2, B, T, 1024, **f32) if len(chunks) == 1 else None     # cleared by t2v_bilstm_bwd
        dgs = []
        stamp('bilstm_bwd_begin')
        for b0, b1, gates, cells, sync in chunks:
            Bc = b1 - b0
            dg_c = dg if dg is not None else torch.empty(2, Bc, T, 1024, **f32)
            dgx = torch.empty(2 * 2 * 2 * 16 * 16 * 256, **f32)        # 8-byte granules: (dir, parity, producer, item, unit)
            _check(lib.t2v_bilstm_bwd(_p(whh), _p(lengths[b0:b1]), _p(dy[b0:b1]), _p(gates), _p(cells), _p(dg_c), _p(dgx),
                                      _p(sync), Bc, T, _stream()), 't2v_bilstm_bwd')
            _err_note('BiLSTM backward', sync[2:3])
            dgs.append(dg_c)
        stamp('bilstm_bwd_end')
        BT = B * T
        if dg is None:
            dg = torch.cat(dgs, 1)
        d0, d1, x2 = dg[0].reshape(BT, 1024), dg[1].reshape(BT, 1024), x.view(BT, -1)
        fork = mark()
        dx = gemm(d0, w_ih.t())
        gemm(d1, w_ih_r.t(), out=dx, accumulate=True)
        dx = dx.view(B, T, -1)
        db0, db1 = colsum(d0), colsum(d1)        # each handed to two inputs (b_ih, b_hh): autograd clones -> this stream
        with side('w', keep=(dg, d0, d1, dy), after=fork):          # weight gradients: deferred-work stream
            z = y.new_zeros(B, 1, 256)
            hp0 = torch.cat((z, y[:, :-1, :256]), 1).reshape(BT, 256)      # h_{t-1} of the forward direction
            hp1 = torch.cat((y[:, 1:, 256:], z), 1).reshape(BT, 256)       # h_{t+1} of the reverse direction
            g = (gemm(d0.t(), x2.t(), out=grad_slot(w_ih)), gemm(d0.t(), hp0.t()),
                 gemm(d1.t(), x2.t(), out=grad_slot(w_ih_r)), gemm(d1.t(), hp1.t()))
        return (dx, None, g[0], g[1], db0, db0, g[2], g[3], db1, db1, None)


def bilstm_check(sync):
    """Raises if a cooperative kernel reported a barrier timeout (forces a device sync; tests only)."""
    if int(sync[2].item()) != 0:
        raise T2VHipError("BiLSTM cooperative kernel timed out on its inter-workgroup barrier")


def colsum(x):
    """sum over the rows of a 2-D fp32 matrix (unit column stride): the `grad.sum(0)` of a bias, on t2v_colsum"""
    lib = _require_gpu(x)
    assert x.dim() == 2 and x.dtype == torch.float32
    if x.stride(1) != 1 and x.shape[1] > 1:
        x = x.contiguous()
    M, N = x.shape
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    nscr = lib.t2v_colsum_scratch_floats(M, N)
    scr = torch.empty(nscr, device=x.device, dtype=torch.float32) if nscr else None
    _check(lib.t2v_colsum(_p(x), x.stride(0) if M > 1 else N, M, N, _p(scr), _p(out), _stream()), 't2v_colsum')
    return out


# ---- gradient slots: FlatAdam keeps every parameter's gradient in one flat arena; a backward that knows the slot of
# its weight writes the gradient GEMM straight into it (autograd then adopts the returned view as `.grad` and
# FlatAdam.gather_grads() finds it already in place) instead of a fresh tensor that is copied into the arena later.
_GRAD_SLOTS = {}


def register_grad_slots(slots):
    """slots: {param.data_ptr(): (flat grads tensor, offset, shape)}; replaces the previous registration"""
    _GRAD_SLOTS.clear()
    _GRAD_SLOTS.update(slots)


def grad_slot(weight):
    """a fresh view of the arena slot that holds d(weight), or None (= let the GEMM allocate) when no slot is
    registered or the parameter already carries a gradient (a second backward before zero_grad must ADD to it)"""
    if not weight.is_leaf or weight.grad is not None:
        return None
    ent = _GRAD_SLOTS.get(weight.data_ptr())
    if ent is None:
        return None
    flat, off, shape = ent
    if tuple(shape) != tuple(weight.shape) or flat.device != weight.device:
        return None
    return flat[off:off + weight.numel()].view(shape)


def _small_grads(params, n, f32):
    """gradient tensors for (gamma, beta, conv bias): their arena slots when registered, else one fresh tensor each"""
    out = []
    for p in params:
        g = grad_slot(p) if p is not None else None
        out.append(torch.empty(n, **f32) if g is None else g)
    return out


def _group_array(groups):
    arr = (_GemmGroup * len(groups))()
    for g, (A, parts) in zip(arr, groups):
        g.A, g.sAi, g.sAk, g.nb = A.data_ptr(), A.stride(0), A.stride(1), len(parts)
        for p, (Bp, out) in enumerate(parts):
            g.B[p], g.sBj[p], g.sBk[p], g.N[p] = Bp.data_ptr(), Bp.stride(0), Bp.stride(1), Bp.shape[0]
            g.C[p], g.ldc[p] = out.data_ptr(), out.stride(0)
    return arr


class GroupedHandOver(object):
    """What a kernel in FRONT of gemm_grouped(groups) needs to start on group `g` (the one-launch reverse pass on decoder_rnn's
    weight gradients, t2v_achain_dw), and what gemm_grouped(groups, handed=this) needs to finish it: the launch's scratch, made
    here; the counter word the first kernel takes tiles from; the test-only cap on those tiles (None: no cap)."""

    def __init__(self, groups, g, counter, accumulate, cap=None):
        lib = load_library()
        assert g == 1 and len(groups) == 2 and len(groups[1][1]) == 2
        M, K = groups[0][0].shape
        self.groups, self.g, self.counter = groups, g, counter
        arr = _group_array(groups)
        off = lib.t2v_gemm_f32_grouped_group_offset(arr, len(groups), M, K, g)
        if off < 0:
            raise T2VHipError("GroupedHandOver: these products do not take the grouped plane launch")
        self.scr = torch.empty(lib.t2v_gemm_f32_grouped_scratch_floats(arr, len(groups), M, K), device=counter.device, dtype=torch.float32)
        self.cap = -1 if cap is None else int(cap)
        (_, out_ih), (_, out_hh) = groups[g][1]
        self.dw = _AchainDw(self.scr.data_ptr() + 4 * off, out_ih.data_ptr(), out_ih.stride(0), out_hh.data_ptr(), out_hh.stride(0),
                            int(bool(accumulate)), self.cap)


def gemm_grouped(groups, accumulate=False, handed=None):
    """groups: [(A (M,K), [(B_p (N_p,K), out_p (M,N_p)), ...]), ...] (at most two groups of at most three parts, one common M and K):
    out_p (+)= A · B_p^T for every part.  Every operand is split (fp32: into its three bf16 planes; bf16_run: rounded to bf16) once, all
    tiles run as ONE launch (t2v_gemm_f32_grouped / t2v_gemm_bf16_grouped); shapes the grouped kernel does not take: the products one by
    one through gemm().  handed: the GroupedHandOver of these groups — an earlier kernel has made one group's planes and some of
    its tiles."""
    lib = _require_gpu(groups[0][0])
    M, K = groups[0][0].shape
    if handed is not None:
        assert handed.groups is groups and not _BF16
        cap = handed.cap if handed.cap >= 0 else 2 ** 31 - 1
        _check(lib.t2v_gemm_f32_grouped_handed(_group_array(groups), len(groups), M, K, int(bool(accumulate)), _p(handed.scr), handed.g,
                                               _p(handed.counter), cap, _stream()), 't2v_gemm_f32_grouped_handed')
        return
    ok = 1 <= len(groups) <= 2
    for A, parts in groups:
        ok = ok and A.shape == (M, K) and A.dtype == torch.float32 and 1 <= len(parts) <= 3
        for Bp, out in parts:
            ok = ok and Bp.shape[1] == K and Bp.dtype == torch.float32 and out.shape == (M, Bp.shape[0]) and out.stride(1) == 1 and Bp.shape[0] % 128 == 0
    if not ok:
        for A, parts in groups:
            for Bp, out in parts:
                gemm(A, Bp, out=out, accumulate=accumulate)
        return
    arr = _group_array(groups)
    size_fn, run_fn = ((lib.t2v_gemm_bf16_grouped_scratch_floats, lib.t2v_gemm_bf16_grouped) if _BF16 else
                       (lib.t2v_gemm_f32_grouped_scratch_floats, lib.t2v_gemm_f32_grouped))
    nscr = size_fn(arr, len(groups), M, K)
    scr = torch.empty(max(nscr, 4), device=groups[0][0].device, dtype=torch.float32)
    _check(run_fn(arr, len(groups), M, K, int(bool(accumulate)), _p(scr), _stream()), 't2v_gemm_grouped')


def set_f32_gemm_mode(x3):
    """True (default): the large fp32 products run as six bf16 MFMAs on exactly 3-way-split operands (fp32-class accuracy, see
    include/t2vae.h: t2v_gemm_f32_set_mode); False: fp32 MFMA only; None: query.  Returns the previous setting."""
    return bool(load_library().t2v_gemm_f32_set_mode(-1 if x3 is None else int(bool(x3))))


def gemm(A, B, bias=None, out=None, relu=False, accumulate=False, p_drop=0.0, seed=0, rng_stream=0, rng_t=0):
    """out[i][j] (+)= sum_k A[i][k] * B[j][k] (+ bias[j]) on the HIP MFMA GEMM; A (M,K), B (N,K) may be any
    2-D strided views (pass W for x·W^T, W.t() for dy·W, dy.t()/x.t() for dy^T·x)."""
    lib = _require_gpu(A, B)
    M, K = A.shape
    N, K2 = B.shape
    assert K == K2 and A.dtype == torch.float32 and B.dtype == torch.float32
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    # `out` may be a column block of a wider row-major matrix (row stride ldc >= N): the weight-gradient GEMMs write
    # the [weight_ih | weight_hh] halves of one product straight into their own tensors
    assert out.shape == (M, N) and out.dtype == torch.float32 and (N == 1 or out.stride(1) == 1)
    ldc = out.stride(0) if M > 1 else max(N, out.stride(0))
    assert ldc >= N and (ldc == N or p_drop == 0.0)
    # skinny deep-K product (a handful of tiles, K = T*B): split K over workgroups, fixed-order partial sum.  Under bf16_run
    # too: the bf16 64x64 kernel has no split-K, and on 8..48 workgroups with K = 6400 these products took 190-200 us each
    # (B = 16 step trace) against 20-30 us on the fp32 split-K kernel — fp32 operands are no loss of accuracy.
    if True:
        nscr = lib.t2v_gemm_splitk_scratch_floats(M, N, K)
        if nscr and _BF16 and ((M + 63) // 64) * ((N + 63) // 64) >= 64:
            nscr = 0        # enough tiles for the bf16 kernels (the LSTM weight gradients go to the 128x128 bf16 GEMM)
        if nscr:
            scr = torch.empty(nscr, device=A.device, dtype=torch.float32)
            _check(lib.t2v_gemm_f32_splitk(_p(A), A.stride(0), A.stride(1), _p(B), B.stride(0), B.stride(1), _p(bias), _p(out),
                                           ldc, M, N, K, int(relu), int(accumulate), float(p_drop), int(seed), int(rng_stream),
                                           int(rng_t), _p(scr), _stream()), 't2v_gemm_f32_splitk')
            return out
    if _BF16:
        # a bf16 kernel on a grid that leaves CUs idle with a deep K (the deferred LSTM weight gradients on the 128x128 tile; the
        # projection, the BiLSTM data / weight gradients on the 64x64 tile): split over k, fixed-order sum of the partials
        nscr = lib.t2v_gemm_bf16_splitk_scratch_floats(M, N, K)
        if nscr:
            scr = torch.empty(nscr, device=A.device, dtype=torch.float32)
            _check(lib.t2v_gemm_bf16_splitk(_p(A), A.stride(0), A.stride(1), _p(B), B.stride(0), B.stride(1), _p(bias), _p(out),
                                            ldc, M, N, K, int(relu), int(accumulate), float(p_drop), int(seed), int(rng_stream),
                                            int(rng_t), _p(scr), _stream()), 't2v_gemm_bf16_splitk')
            return out
    fn = lib.t2v_gemm_bf16 if _BF16 else lib.t2v_gemm_f32
    _check(fn(_p(A), A.stride(0), A.stride(1), _p(B), B.stride(0), B.stride(1), _p(bias), _p(out), ldc,
              M, N, K, int(relu), int(accumulate), float(p_drop), int(seed), int(rng_stream),
              int(rng_t), _stream()), 't2v_gemm_bf16' if _BF16 else 't2v_gemm_f32')
    return out


class LinearHIP(torch.autograd.Function):
    """y = dropout(relu?(x·W^T + b)) over the last dimension of x, on t2v_gemm_f32 (forward and both
    gradients).  The dropout mask is regenerated in the backward from (seed, stream, t)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, p_drop, seed, rng_stream, rng_t):
        _require_gpu(x, weight)
        x2 = x.reshape(-1, x.shape[-1])
        x2 = x2 if x2.dtype == torch.float32 else x2.float()
        y = gemm(x2, weight, bias, relu=relu, p_drop=p_drop, seed=seed, rng_stream=rng_stream, rng_t=rng_t)
        ctx.save_for_backward(x2, weight, y if (relu or p_drop > 0) else None)
        ctx.cfg = (x.shape, bool(relu), float(p_drop), bias is not None)
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, y = ctx.saved_tensors
        xshape, relu, p, has_bias = ctx.cfg
        dy2 = _f32c(dy.reshape(-1, weight.shape[0]))
        if relu or p > 0:
            # y already carries relu and the 1/(1-p) scaling: d/dpre = dy * [y != 0] * scale
            scale = 1.0 / (1.0 - p) if p > 0 else 1.0
            masked = torch.empty_like(dy2)
            _check(load_library().t2v_gemm_epilogue_bwd(_p(dy2), _p(y), _p(masked), dy2.numel(), scale, _stream()),
                   't2v_gemm_epilogue_bwd')
            dy2 = masked
        fork = mark()
        dx = gemm(dy2, weight.t()) if ctx.needs_input_grad[0] else None          # (N,K) = dy · W
        # Deferral rule (also in the other nodes): only a gradient that travels STRAIGHT into a leaf's AccumulateGrad as
        # the sole reference (autograd adopts the tensor without touching its data) may be produced on the deferred-work
        # stream.  Anything autograd may read on the node's own stream before the engine's join — a tensor handed to two
        # inputs (cloned), a gradient that flows on through Cat/Add/Slice nodes — is produced on the node's stream.
        if weight.is_leaf:
            with side('w', keep=(dy2, x2), after=fork):     # weight gradient: deferred-work stream of the engine
                dw = gemm(dy2.t(), x2.t(), out=grad_slot(weight))                  # (M,K) = dy^T · x
        else:
            dw = gemm(dy2.t(), x2.t())
        db = colsum(dy2) if has_bias else None
        return (dx.view(xshape) if dx is not None else None), dw, db, None, None, None, None, None


# reference-encoder convolutions as im2col + batched GEMM (T2V_CONV2D_GEMM=0: the direct-form kernels)
CONV2D_GEMM = os.environ.get('T2V_CONV2D_GEMM', '1') != '0'


class Conv2dBNReLU(torch.autograd.Function):
    """relu(BatchNorm2d(Conv2d 3x3 s2 p1 (x [+ CoordConv channels]))) — one layer of the reference encoder
    (reference modules.py:68-71) on the direct-form HIP conv + the per-channel BN kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, training, coord):
        lib = _require_gpu(x, weight)
        x = _f32c(x)
        B, Cx, Hh, Ww = x.shape
        Cout = weight.shape[0]
        Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
        f32 = dict(device=x.device, dtype=torch.float32)
        w = weight.contiguous()
        y = torch.empty(B, Cout, Ho, Wo, **f32)
        gscr = None
        if CONV2D_GEMM:      # im2col + batched MFMA GEMM (the im2col matrix stays in gscr for the backward pass)
            gscr = torch.empty(lib.t2v_conv2d_s2_gemm_scratch_floats(B, Cx, Hh, Ww, Cout, int(coord)), **f32)
            _check(lib.t2v_conv2d_s2_fwd_gemm(_p(x), _p(w), _p(bias), _p(y), _p(gscr), B, Cx, Hh, Ww, Cout, int(coord), _stream()),
                   't2v_conv2d_s2_fwd_gemm')
        else:
            _check(lib.t2v_conv2d_s2_fwd(_p(x), _p(w), _p(bias), _p(y), B, Cx, Hh, Ww, Cout, int(coord), _stream()),
                   't2v_conv2d_s2_fwd')
        mean = torch.empty(Cout, **f32) if training else None
        rstd = torch.empty(Cout, **f32) if training else None
        out = torch.empty_like(y)
        _check(lib.t2v_bn_act_fwd(_p(y), None, 0, _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(mean),
                                  _p(rstd), _p(out), B, Cout, Ho * Wo, ACT_RELU, int(bool(training)), 0.0, 0.1, 1e-5,
                                  0, 0, 0, _stream()), 't2v_bn_act_fwd')
        ctx.keep = (x, w, y, mean, rstd, gamma, beta)
        ctx.gscr = gscr
        ctx.running = (running_mean, running_var)
        ctx.small = (gamma, beta, bias)
        ctx.cfg = (B, Cx, Hh, Ww, Cout, Ho, Wo, int(coord), bool(training))
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = load_library()
        x, w, y, mean, rstd, gamma, beta = ctx.keep
        B, Cx, Hh, Ww, Cout, Ho, Wo, coord, training = ctx.cfg
        bn_bwd = lib.t2v_bn_act_bwd
        if not training:        # eval-mode BatchNorm2d: running statistics are constants
            mean, rstd = ctx.running[0], torch.rsqrt(ctx.running[1] + 1e-5)
            bn_bwd = lib.t2v_bn_act_bwd_eval
        f32 = dict(device=x.device, dtype=torch.float32)
        dout = dout.contiguous()
        dy = torch.empty_like(y)
        dgamma, dbeta, dbias = _small_grads(ctx.small, Cout, f32)
        _check(bn_bwd(_p(y), _p(dout), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dy), _p(dgamma),
                      _p(dbeta), _p(dbias), B, Cout, Ho * Wo, ACT_RELU, 0.0, 0, 0, 0, _stream()), 't2v_bn_act_bwd')
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        if ctx.gscr is not None:
            _check(lib.t2v_conv2d_s2_bwd_gemm(_p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(ctx.gscr), B, Cx, Hh, Ww, Cout, coord,
                                              _stream()), 't2v_conv2d_s2_bwd_gemm')
            ctx.gscr = None
        else:
            nscr = lib.t2v_conv2d_s2_dw_scratch_floats(B, Cx, Hh, Ww, Cout, coord)
            scr = torch.empty(nscr, **f32) if nscr else None
            _check(lib.t2v_conv2d_s2_bwd(_p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(scr), B, Cx, Hh, Ww, Cout, coord,
                                         _stream()), 't2v_conv2d_s2_bwd')
        return dx, dw, dbias, dgamma, dbeta, None, None, None, None


class GRULast(torch.autograd.Function):
    """Last hidden state of nn.GRU(batch_first) (reference modules.py:78-80)."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh):
        lib = _require_gpu(x, w_ih)
        B, T, I = x.shape
        f32 = dict(device=x.device, dtype=torch.float32)
        x2 = _f32c(x).view(B * T, I)
        gi = gemm(x2, w_ih, b_ih)                                   # (B*T,768)
        hs = torch.empty(B, T + 1, 256, **f32)
        gsave = torch.empty(B, T, 4, 256, **f32)
        whh = w_hh.contiguous()
        xchg = torch.empty(2 * 16 * 768, **f32)                       # exchange buffer (forward uses 2*16*256 of it)
        syncs = []
        gi3 = gi.view(B, T, 768)
        for b0 in range(0, B, MAX_DEC_B):          # 16 sequences per cooperative launch; rows of a chunk are contiguous
            b1 = min(B, b0 + MAX_DEC_B)
            sync = torch.empty(2, device=x.device, dtype=torch.int32)
            _check(lib.t2v_gru_fwd(_p(gi3[b0:b1]), _p(whh), _p(b_hh), _p(hs[b0:b1]), _p(gsave[b0:b1]), _p(xchg), _p(sync),
                                   b1 - b0, T, _stream()), 't2v_gru_fwd')
            _err_note('GRU forward', sync[1:2])
            syncs.append(sync)
        ctx.keep = (x2, w_ih, whh, hs, gsave, xchg, syncs)
        ctx.dims = (B, T, I)
        return hs[:, T].clone()

    @staticmethod
    def backward(ctx, dh):
        lib = load_library()
        x2, w_ih, whh, hs, gsave, xchg, syncs = ctx.keep
        B, T, I = ctx.dims
        f32 = dict(device=x2.device, dtype=torch.float32)
        dgi, dgh = torch.empty(B, T, 768, **f32), torch.empty(B, T, 768, **f32)
        dh = dh.contiguous()
        for i, b0 in enumerate(range(0, B, MAX_DEC_B)):
            b1 = min(B, b0 + MAX_DEC_B)
            _check(lib.t2v_gru_bwd(_p(whh), _p(hs[b0:b1]), _p(gsave[b0:b1]), _p(dh[b0:b1]), _p(dgi[b0:b1]), _p(dgh[b0:b1]),
                                   _p(xchg), _p(syncs[i]), b1 - b0, T, _stream()), 't2v_gru_bwd')
            _err_note('GRU backward', syncs[i][1:2])
        dgi2, dgh2 = dgi.view(B * T, 768), dgh.view(B * T, 768)
        fork = mark()
        dx = gemm(dgi2, w_ih.t()).view(B, T, I)
        with side('w', keep=(dgi, dgh, hs, x2), after=fork):
            hprev = hs[:, :T].reshape(B * T, 256)
            g = (gemm(dgi2.t(), x2.t()), gemm(dgh2.t(), hprev.t()))
        return (dx,) + g + (colsum(dgi2), colsum(dgh2))


def refenc_heights(n_frames, n_layers):
    """per-item input heights of the reference encoder's layers, host side: row 0 = the frame counts, row l + 1 =
    (row l - 1) // 2 + 1 (a 3x3 stride-2 pad-1 convolution); the last row is the GRU's step count"""
    h = [[int(x) for x in n_frames]]
    for _ in range(n_layers):
        h.append([(x - 1) // 2 + 1 for x in h[-1]])
    return h


def refenc_ragged(mel, n_frames, layers, gru):
    """Eval-mode ReferenceEncoder over a ragged batch, no autograd: row b is what the encoder gives for
    mel[b:b+1, :, :n_frames[b]] alone.  mel: (B, n_mels, T) CUDA float32, anything past an item's frames is never read;
    n_frames: host ints, already checked (2 <= n <= T).  layers: per conv layer (weight, bias, gamma, beta, running_mean,
    running_var), layer 0 the CoordConv inner conv; gru: (w_ih, w_hh, b_ih, b_hh).  Returns the last GRU states (B, 256)
    at each item's own step count.  Same conv form as Conv2dBNReLU (CONV2D_GEMM), BatchNorm2d eval + ReLU on t2v_bn_act_fwd."""
    lib = _require_gpu(mel)
    x = _f32c(mel)
    B, n_mels, T = x.shape
    f32 = dict(device=x.device, dtype=torch.float32)
    heights = torch.tensor(refenc_heights(n_frames, len(layers)), dtype=torch.int32).to(x.device)    # one upload
    Hh, Ww, Cx = T, n_mels, 1
    for i, (weight, bias, gamma, beta, running_mean, running_var) in enumerate(layers):
        coord, tstride = int(i == 0), (T if i == 0 else 0)          # layer 0 gathers the reinterpreted rows from the mel
        Cout = weight.shape[0]
        Ho, Wo = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
        w = _f32c(weight.detach())
        y = torch.empty(B, Cout, Ho, Wo, **f32)
        hlen = heights[i]
        if CONV2D_GEMM:
            scr = torch.empty(lib.t2v_conv2d_s2_gemm_ragged_scratch_floats(B, Cx, Hh, Ww, Cout, coord), **f32)
            _check(lib.t2v_conv2d_s2_fwd_gemm_ragged(_p(x), _p(w), _p(bias), _p(y), _p(scr), _p(hlen), B, Cx, Hh, Ww, Cout, coord,
                                                     tstride, _stream()), 't2v_conv2d_s2_fwd_gemm_ragged')
        else:
            _check(lib.t2v_conv2d_s2_fwd_ragged(_p(x), _p(w), _p(bias), _p(y), _p(hlen), B, Cx, Hh, Ww, Cout, coord, tstride,
                                                _stream()), 't2v_conv2d_s2_fwd_ragged')
        x = torch.empty_like(y)
        _check(lib.t2v_bn_act_fwd(_p(y), None, 0, _p(gamma), _p(beta), _p(running_mean), _p(running_var), None, None, _p(x),
                                  B, Cout, Ho * Wo, ACT_RELU, 0, 0.0, 0.1, 1e-5, 0, 0, 0, _stream()), 't2v_bn_act_fwd')
        Hh, Ww, Cx = Ho, Wo, Cout
    steps = heights[len(layers)]
    seq = x.transpose(1, 2).contiguous().view(B * Hh, Cx * Ww)     # (B, steps_max, C*W) as ReferenceEncoder.forward
    w_ih, w_hh, b_ih, b_hh = gru
    gi = gemm(seq, w_ih.detach(), b_ih.detach()).view(B, Hh, 768)
    hs = torch.empty(B, Hh + 1, 256, **f32)
    h_last = torch.empty(B, 256, **f32)
    whh = _f32c(w_hh.detach())
    xchg = torch.empty(2 * 16 * 256, **f32)
    for b0 in range(0, B, MAX_DEC_B):          # 16 sequences per cooperative launch, as GRULast
        b1 = min(B, b0 + MAX_DEC_B)
        sync = torch.empty(2, device=x.device, dtype=torch.int32)
        _check(lib.t2v_gru_fwd_len(_p(gi[b0:b1]), _p(whh), _p(b_hh), _p(hs[b0:b1]), None, _p(xchg), _p(sync), _p(steps[b0:b1]),
                                   _p(h_last[b0:b1]), b1 - b0, Hh, _stream()), 't2v_gru_fwd_len')
        _err_note('GRU forward', sync[1:2])
    return h_last


def guided_attention(align, in_lengths, out_lengths, sigma=0.4):
    """Guided attention loss of the alignments (B, T, T_in), read in whatever strides they have (csrc/guided_attention.hip):
    returns (L, G) — L the loss as a 0-d tensor, G = dL/dalign as a (B, T, T_in) view of contiguous (T, B, T_in) storage, the layout
    DecoderCore.backward hands to the reverse kernels without a copy.  Nothing is read back: capturable."""
    lib = _require_gpu(align)
    if align.dim() != 3 or align.dtype != torch.float32:
        raise T2VHipError("guided_attention takes float32 alignments (B, T, T_in)")
    B, T, T_in = align.shape
    dev = align.device
    lens = [t.to(device=dev, dtype=torch.int64).contiguous() for t in (in_lengths, out_lengths)]
    if lens[0].numel() != B or lens[1].numel() != B:
        raise T2VHipError("guided_attention: one input length and one output length per item")
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    G = torch.empty(T, B, T_in, device=dev, dtype=torch.float32)
    part = torch.empty(lib.t2v_guided_attention_part_doubles(B, T), device=dev, dtype=torch.float64)
    sb, st, sj = align.stride()
    _check(lib.t2v_guided_attention(_p(align), sb, st, sj, _p(lens[0]), _p(lens[1]), _p(loss), _p(G), _p(part), B, T, T_in,
                                    float(sigma), _stream()), 't2v_guided_attention')
    return loss[0], G.permute(1, 0, 2)


class GuidedAttention(torch.autograd.Function):
    """guided_attention as a differentiable scalar: the gradient comes with the value, the backward is one multiply."""

    @staticmethod
    def forward(ctx, align, in_lengths, out_lengths, sigma):
        loss, G = guided_attention(align.detach(), in_lengths, out_lengths, sigma)
        ctx.G = G
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return ctx.G * dloss, None, None, None


class VAELoss(torch.autograd.Function):
    """Tacotron2Loss_VAE value + gradient in one HIP launch (reference loss_function.py:27-44)."""
    _scratch = {}

    @staticmethod
    def forward(ctx, mel, post, gate, mu, logvar, mel_t, gate_t, kl_weight):
        lib = _require_gpu(mel, post, gate, mu, logvar)
        dev = mel.device
        key = str(dev)
        if key not in VAELoss._scratch:
            VAELoss._scratch[key] = (torch.empty(192, device=dev), torch.zeros(1, device=dev, dtype=torch.int32))
        part, ticket = VAELoss._scratch[key]
        mel, post, gate, mu, logvar = (_f32c(t) for t in (mel, post, gate, mu, logvar))
        mel_t, gate_t = _f32c(mel_t), _f32c(gate_t)
        out = torch.empty(4, device=dev, dtype=torch.float32)
        sp = step_params(create=False)
        if sp is not None:       # the kernel reads the KL weight from the device record once one is installed
            sp.set(kl_weight=kl_weight)
            sp.upload()
        grads = [torch.empty_like(t) for t in (mel, post, gate, mu, logvar)]
        _check(lib.t2v_loss_fwd_bwd(_p(mel), _p(post), _p(mel_t), _p(gate), _p(gate_t), _p(mu), _p(logvar),
                                    *[_p(g) for g in grads], _p(part), _p(out), _p(ticket), mel.numel(),
                                    gate.numel(), mu.numel(), float(kl_weight), _stream()), 't2v_loss_fwd_bwd')
        ctx.grads = grads
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, dtotal, _dout):
        g = torch._foreach_mul(ctx.grads, dtotal)       # one multi-tensor launch instead of five
        return (g[0], g[1], g[2], g[3], g[4], None, None, None)


class KLMonitor(object):
    """Running per-dimension record of the posterior over the training batches of a window, kept by the loss launch itself
    (csrc/kl_control.hip): 3 * dims + 2 doubles on the device — rows seen, launches seen, and per dimension the running mean of mu, its
    M2 and the sum of the KL.  The buffer's address is fixed for the monitor's life, so a captured step keeps updating it."""

    def __init__(self, dims, device='cuda'):
        dims = int(dims)
        if not 1 <= dims <= 256:
            raise T2VHipError("KLMonitor: 1..256 latent dimensions, got %d" % dims)
        self.dims = dims
        self.buf = torch.zeros(3 * dims + 2, device=device, dtype=torch.float64)

    def reset(self):
        self.buf.zero_()        # a memset on the current stream: ordered with the launches around it, no host round trip

    def read(self):
        """{'n': rows seen, 'launches', 'mean', 'm2', 'active_units', 'kl_per_dim'} of the window so far (synchronises).
        active_units: dimensions whose variance of mu, M2 / (n - 1), exceeds latent_scores.ACTIVE_THRESHOLD (Burda et al.);
        kl_per_dim: mean nats per utterance, (dims,) fp64."""
        from latent_scores import ACTIVE_THRESHOLD
        v = self.buf.cpu().numpy()
        D, n = self.dims, int(v[0])
        mean, m2, skl = v[2:2 + D], v[2 + D:2 + 2 * D], v[2 + 2 * D:2 + 3 * D]
        return {'n': n, 'launches': int(v[1]), 'mean': mean.copy(), 'm2': m2.copy(),
                'active_units': int((m2 / (n - 1) > ACTIVE_THRESHOLD).sum()) if n > 1 else 0,
                'kl_per_dim': skl / n if n > 0 else skl.copy()}


class VAELossKLC(torch.autograd.Function):
    """Tacotron2Loss_VAE with free bits, a KL capacity target and the monitor update, value + gradient in one HIP launch
    (csrc/kl_control.hip).  Returns (total, out8): out8 = [total, recon, raw KL, w, K', T, floored dimensions, s]."""

    @staticmethod
    def forward(ctx, mel, post, gate, mu, logvar, mel_t, gate_t, kl_weight, free_bits, capacity, monitor):
        lib = _require_gpu(mel, post, gate, mu, logvar)
        dev = mel.device
        key = str(dev)
        if key not in VAELoss._scratch:
            VAELoss._scratch[key] = (torch.empty(192, device=dev), torch.zeros(1, device=dev, dtype=torch.int32))
        part, ticket = VAELoss._scratch[key]
        mel, post, gate, mu, logvar = (_f32c(t) for t in (mel, post, gate, mu, logvar))
        mel_t, gate_t = _f32c(mel_t), _f32c(gate_t)
        if mu.dim() != 2 or mu.shape != logvar.shape:
            raise T2VHipError("VAELossKLC takes mu and logvar of one (B, D) shape")
        B, D = mu.shape
        if monitor is not None and (monitor.dims != D or monitor.buf.device != dev):
            raise T2VHipError("VAELossKLC: the monitor was made for %d dimensions on %s" % (monitor.dims, monitor.buf.device))
        out = torch.empty(8, device=dev, dtype=torch.float32)
        sp = step_params(create=False)
        if sp is not None:       # the kernel reads the KL weight from the device record once one is installed
            sp.set(kl_weight=kl_weight)
            sp.upload()
        grads = [torch.empty_like(t) for t in (mel, post, gate, mu, logvar)]
        _check(lib.t2v_loss_fwd_bwd_klc(_p(mel), _p(post), _p(mel_t), _p(gate), _p(gate_t), _p(mu), _p(logvar),
                                        *[_p(g) for g in grads], _p(part), _p(out), _p(ticket),
                                        _p(monitor.buf) if monitor is not None else None, mel.numel(), gate.numel(), B, D,
                                        float(kl_weight), float(free_bits), float(capacity), _stream()), 't2v_loss_fwd_bwd_klc')
        ctx.grads = grads
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, dtotal, _dout):
        g = torch._foreach_mul(ctx.grads, dtotal)       # VAELoss's one multi-tensor multiply
        return (g[0], g[1], g[2], g[3], g[4], None, None, None, None, None, None)
