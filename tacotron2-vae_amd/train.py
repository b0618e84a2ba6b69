"""Training driver for the MI355X Tacotron2-VAE path.

Same CLI flags, function names and checkpoint dict as the reference's train.py
(`load_model` 80-89, `warm_start_model` 92-97, `load_checkpoint` 100-110, `save_checkpoint`
113-119, `validate` 122-147, `train` 150-250, argparse 252-285); the loop body is re-hosted on
the HIP kernels: flat-arena gradients, one RCCL all-reduce on the arena, fused clip+Adam.
Launch multi-GPU runs as `python -m torch.distributed.run --nproc-per-node N train.py ...
--hparams=distributed_run=True` (replaces multiproc.py); the reference's `--n_gpus/--rank`
flags still work with hparams.dist_url.
"""
import argparse
import math
import os
import time

import torch
import torch.distributed as dist

import distributed as t2v_dist
from graph_cache import CAPTURE, COMPARE, REPLAY, GraphCache
from hparams import create_hparams
from loss_function import Tacotron2Loss_VAE
from model import BatchLayout, Tacotron2
from optim import FlatAdam


def load_model(hparams):
    """reference train.py:80-89.  fp16_run (apex-style fp16, fp16_optimizer.py / loss_scaler.py) is replaced by
    hparams.bf16_run and is rejected here instead of silently running something else.  The precision switch is
    process-wide (t2v_hip.set_bf16): the last load_model() call decides."""
    if not torch.cuda.is_available():
        raise RuntimeError("load_model needs a GPU: the Tacotron2-VAE path here is HIP-only")
    if hparams.fp16_run:
        raise NotImplementedError("fp16_run (apex-style fp16 + loss scaling) is replaced by bf16_run=True: "
                                  "bf16 MFMA operands with fp32 master weights, no loss scaling needed")
    import t2v_hip
    t2v_hip.set_bf16(bool(getattr(hparams, 'bf16_run', False)))
    model = Tacotron2(hparams).cuda()
    if hparams.distributed_run:
        model = t2v_dist.apply_gradient_allreduce(model)
    return model


def warm_start_model(checkpoint_path, model, optimizer=None):
    """reference train.py:92-97.  optimizer: a FlatAdam that keeps a weight average seeds it from the loaded weights."""
    assert os.path.isfile(checkpoint_path)
    print("Warm starting model from checkpoint '{}'".format(checkpoint_path))
    ckpt = torch.load(checkpoint_path, map_location='cpu')
    model.load_state_dict(ckpt['state_dict'])
    if getattr(optimizer, 'ema', None) is not None:
        optimizer.reset_ema()
    return model


def load_checkpoint(checkpoint_path, model, optimizer):
    assert os.path.isfile(checkpoint_path)
    print("Loading checkpoint '{}'".format(checkpoint_path))
    ckpt = torch.load(checkpoint_path, map_location='cpu')
    model.load_state_dict(ckpt['state_dict'])
    optimizer.load_state_dict(ckpt['optimizer'])
    if getattr(optimizer, 'ema', None) is not None:
        if 'ema_state_dict' in ckpt:
            optimizer.load_ema_state_dict(ckpt['ema_state_dict'])
        else:       # (load_state_dict above already made the shadow a copy of the loaded weights)
            print("Checkpoint '{}' holds no 'ema_state_dict': the weight average starts from its weights".format(checkpoint_path))
    print("Loaded checkpoint '{}' from iteration {}".format(checkpoint_path, ckpt['iteration']))
    return model, optimizer, ckpt['learning_rate'], ckpt['iteration']


def save_checkpoint(model, optimizer, learning_rate, iteration, filepath):
    """dict layout of reference train.py:116-119 (tensors cloned out of the arena).  An optimiser that keeps a weight
    average (hparams.ema_decay > 0) adds 'ema_state_dict' (the keys of 'state_dict', live parameters averaged) and
    'ema': {'decay', 'warmup'}; without one the dict is the reference's four keys and nothing else."""
    print("Saving model and optimizer state at iteration {} to {}".format(iteration, filepath))
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ckpt = {'iteration': iteration, 'state_dict': state, 'optimizer': optimizer.state_dict(),
            'learning_rate': learning_rate}
    if getattr(optimizer, 'ema', None) is not None:
        ckpt['ema_state_dict'] = optimizer.ema_state_dict(model)
        ckpt['ema'] = {'decay': optimizer.ema_decay, 'warmup': optimizer.ema_warmup}
    torch.save(ckpt, filepath)


def t2v_hip_check():
    import t2v_hip
    t2v_hip.check_async_errors()


class TrainEngine(object):
    """One rank's training state: model + criterion + flat-arena optimiser (+ arena all-reduce).

    graph=True (hparams.graph_step): the whole iteration after the H2D copies — forward, loss, backward, gradient
    gather, clip + Adam — is captured ONCE per input shape into a HIP graph and replayed; everything that changes from
    step to step (dropout epoch, learning rate, Adam bias corrections, KL weight) lives in a 32-byte device record the
    kernels read at run time (t2v_hip.StepParams).  That removes the ~21 ms of host work (1 900 launches, autograd,
    allocator) a step otherwise needs, which is more than the GPU time of the step.  Shapes that keep changing (ragged
    koemo batches without bucketing) simply run eagerly: a shape is captured the third time it is seen."""

    GRAPH_AFTER = 2          # eager executions of a shape before it is captured (allocator / lazy-init warm-up)
    MAX_GRAPHS = 8
    _test_after_replay = None    # tests: called with the span of every replayed graph (a time-out inside a REPLAY)

    # what the graph cache knows, under the names the benchmark, the tools and the tests read
    graph_fallbacks = property(lambda self: self._cache.fallbacks)
    graph_watchdog = property(lambda self: self._cache.watchdog, lambda self, on: setattr(self._cache, 'watchdog', bool(on)))
    _graphs = property(lambda self: self._cache.live())             # shape key -> Entry, least recently replayed first
    _no_graph = property(lambda self: self._cache.verdicts())       # shape key -> (replay ms, eager ms) of a graph that was dropped

    def __init__(self, hparams, world_size=1, graph=None, force_dist=False):
        import t2v_hip
        self._host_threads = t2v_hip.limit_host_threads()
        self.hparams = hparams
        self.model = load_model(hparams)
        self.criterion = Tacotron2Loss_VAE(hparams)
        # hparams.kl_monitor, or a free-bits / capacity run: the training loss launch keeps a per-dimension record of the posterior.
        # One buffer per engine, made before any capture: its address is part of the captured step
        self.kl_monitor = None
        if getattr(hparams, 'kl_monitor', False) or self.criterion.kl_control:
            self.kl_monitor = self.criterion.monitor = t2v_hip.KLMonitor(hparams.z_latent_dim)
        self.optimizer = FlatAdam(self.model, lr=hparams.learning_rate, weight_decay=hparams.weight_decay,
                                  grad_clip_thresh=hparams.grad_clip_thresh, world_size=world_size,
                                  ema_decay=getattr(hparams, 'ema_decay', 0.0), ema_warmup=getattr(hparams, 'ema_warmup', True))
        self.allreduce = None
        if world_size > 1 or force_dist:      # force_dist: 1-rank RCCL group (tests of the launch path on one GPU)
            named, offs = self.optimizer.arena_layout()
            model = self.model
            # bf16_run exchanges bf16 gradients (57.7 MB per step instead of 115.5 MB) unless fp32_allreduce
            wire = (torch.bfloat16 if getattr(hparams, 'bf16_run', False) and not getattr(hparams, 'fp32_allreduce', False)
                    else None)
            self.allreduce = t2v_dist.OverlappedArenaAllReduce(
                named, offs, self.optimizer.grads_for_allreduce(), force=bool(force_dist),
                side_streams=lambda: self.overlap.streams(),
                gather=self.optimizer.gather_grads, wire_dtype=wire, tail=self.optimizer.poison_slot().numel())
        self.use_graph = bool(getattr(hparams, 'graph_step', False) if graph is None else graph)
        # multi-rank graph mode: forward + backward + gradient gather replay as ONE graph, then the whole gradient arena
        # crosses xGMI in one eager all-reduce and the fused clip + Adam runs eagerly (2 launches).  The hook-issued
        # bucket overlap of the eager engine is given up for it: an eager step is host-bound (1 860 launches: 23-32 ms
        # depending on the host), the exposed all-reduce of 115 MB costs well under 1 ms
        self.graph_ddp = self.use_graph and self.allreduce is not None
        # which shapes replay a captured graph and which run eagerly, replay watchdog included (T2V_GRAPH_WATCHDOG=0 switches it off)
        self._cache = GraphCache(lambda: torch.cuda.Event(enable_timing=True), t2v_hip.err_release, self.GRAPH_AFTER, self.MAX_GRAPHS,
                                 watchdog=os.environ.get('T2V_GRAPH_WATCHDOG', '1') != '0')
        self._compare_key = None    # shape whose eager comparison step this step is (never outlives the step)
        self._calib_want = False    # multi-rank graph mode, comparison step: _body marks the end of the timed region in _calib_end
        self._calib_end = None
        self._eager_events = []     # end events of the last two eager steps
        self._test_replay_drag_us = 0   # tests: a kernel that holds 8 workgroups for this long behind every probed replay
        # (round 6, T2V_MAIN_PRIO=-1 — the higher of the two stream priorities for this stream — measured: alone it buys the bf16 step
        # 12.34 -> 12.28 ms and the fp32 step nothing, but the THIRD engine of one process (bench.py's secondary bf16 leg) then replays at
        # 14.15 ms instead of 12.32: another cliff of the graph executor's queue assignment.  The default stays 0.)
        # graph mode: EVERY step of this engine (the eager warm-up ones too) runs on one dedicated stream — autograd's
        # AccumulateGrad nodes remember the stream of their first backward, and a capture that has to synchronise with
        # the legacy default stream is illegal
        self._stream = torch.cuda.Stream(priority=int(os.environ.get('T2V_MAIN_PRIO', '0'))) if self.use_graph else None
        # this engine's device-side step record (dropout epoch, lr, Adam bias corrections, KL weight): bound to the
        # engine's own stream when it has one, so that two engines in one process never share a record
        self.step_params = t2v_hip.step_params(fresh=True, stream=self._stream)
        self.optimizer.step_params = self.step_params
        # round 4: the side streams of this engine's step (reference-encoder branch; deferred work = every weight gradient,
        # Prenet -> gpre).  Created before the first eager step; kernels launched there read the engine's step record too
        self.overlap = t2v_hip.Overlap()
        self.step_params.bind(extra=self.overlap.streams())
        self._err_mark = 0
        self._err_span = None       # ledger block of the graph that was just replayed (multi-rank graph engine: the poison source)
        self._bn_snap = self._bn_bufs = None
        self.recoveries = 0
        # graph engine: the forward pass of a step runs on SHADOW leaves (p.detach().requires_grad_(): same storage, own
        # autograd identity) that only this engine ever touches.  An autograd leaf's gradient sink (AccumulateGrad node)
        # keeps the stream that was current when it was created, and the engine routes gradients to it on that stream
        # even when torch.autograd.grad only captures them there.  A forward pass the caller once ran on another stream
        # with its outputs still alive (evaluate, then train) would therefore pull the legacy default stream into the
        # capture — which kills the process on this stack (found with tests/test_bf16_gpu.py under graph_step=True).
        self._shadow = self._shadow_live = None
        if self.use_graph:
            with torch.cuda.stream(self._stream):
                self._shadow = {n: p.detach().requires_grad_(True) for n, p in self.model.named_parameters()}
            self._shadow_live = [self._shadow[n] for n, _ in self.optimizer.arena_layout()[0]]
        self.model.train()
        # (the first BatchNorm snapshot for recover() is taken at the top of the FIRST step, not here: train() builds the engine and
        # only then loads the checkpoint / warm start — a snapshot from construction time would hold freshly initialised statistics
        # and a time-out on the first step after a resume would copy them over the loaded ones)

    def close(self):
        """unbind this engine's device-side step record from its streams (torch's pooled stream handles are reused)"""
        import t2v_hip
        sp, self.step_params = self.step_params, None
        if sp is not None:
            t2v_hip.drop_step_params(sp)
        self._cache.clear()         # (the graphs' error-ledger blocks go back to the free list)
        prev, self._host_threads = getattr(self, '_host_threads', None), None
        if prev is not None and prev > torch.get_num_threads():
            torch.set_num_threads(prev)         # the host-thread cap belonged to this engine's loop

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream_context(self):
        """`with engine.stream_context():` around the training loop makes the engine's stream the current one, so a step
        needs no hand-over with the caller's stream (an event round trip through the legacy default stream costs
        ≈1.7 ms per step on this stack — measured, tools/graph_probe.py).  No-op for an eager engine."""
        import contextlib
        if self._stream is None:
            return contextlib.nullcontext()

        @contextlib.contextmanager
        def ctx():
            # Round 5 (found by tools/dbg/fuzz_engine.py): the engine's stream is a non-blocking one — it does NOT order itself behind
            # the legacy default stream.  Whatever the caller issued there so far (parameter initialisation, load_state_dict, the
            # optimiser's arena copy, an eps_override) has to be finished before the first step reads it: without this wait the very
            # first step of an engine that is stepped right after its construction could read half-initialised weights (one run in
            # two on a small batch: loss 36.57 instead of 36.31, gradient norm 1e8, NaN from the second step on).  And the other way
            # round on exit: the caller's stream waits for the steps before it reads the weights (checkpoint, validation).
            outer = torch.cuda.current_stream()
            self._stream.wait_stream(outer)
            with torch.cuda.stream(self._stream):
                yield
            outer.wait_stream(self._stream)
        return ctx()

    # -- forward + backward + gradient gather (no collective, no optimiser): what a multi-rank engine captures
    def _body_fb(self, x, y, iteration):
        import t2v_hip
        opt = self.optimizer
        opt.zero_grad()
        t2v_hip.stamp('step_begin')
        y_pred = self._forward(x)
        loss, recon, kl, w = self.criterion(y_pred, y, iteration, lengths=(x[1], x[4]))
        t2v_hip.stamp('loss_end')
        self._backward(loss)
        t2v_hip.stamp('bwd_main_end')
        self.overlap.join()         # weight gradients were produced on the deferred-work stream
        opt.gather_grads()
        t2v_hip.stamp('grads_ready')
        return loss.detach(), recon.detach(), kl.detach()

    def _forward(self, x):
        if self._shadow is None:
            return self.model(x)
        return torch.func.functional_call(self.model, self._shadow, (x,))

    def _backward(self, loss):
        """graph engine: gradients of the shadow leaves through torch.autograd.grad (the big weight gradients are still
        written straight into the arena by the backward kernels: a shadow shares its parameter's storage, so
        t2v_hip.grad_slot finds the slot); `.grad` of the real parameters is set by hand so gather_grads() finds them."""
        if self._shadow is None:
            loss.backward()
            return
        grads = torch.autograd.grad(loss, self._shadow_live, allow_unused=True)
        for p, g in zip(self.optimizer.live_params(), grads):
            p.grad = g

    def _reduce_and_step(self, out, no_grad=None):
        """multi-rank graph mode, after the replay: one all-reduce of the arena, then clip + Adam (1/world folded in).
        no_grad: the live parameters that had no gradient when this graph was captured (FlatAdam skips them like
        torch.optim.Adam does; gather_grads() only runs at capture time, so the set travels with the graph)."""
        self._poison()
        self.allreduce.reduce_all()
        if no_grad is not None:
            self.optimizer._no_grad = list(no_grad)
        self.optimizer.mark_gathered()
        self.optimizer.guard = self._guard_words()
        grad_norm = self.optimizer.step()
        return out[0], out[1], out[2], grad_norm

    # -- one iteration, eager
    def _body(self, x, y, iteration):
        if self.graph_ddp:
            # eager warm-up / fallback step of the multi-rank graph engine: the SAME single whole-arena all-reduce as a
            # replayed step.  Ranks choose replay-or-eager from their own batch-shape history (ragged batches: every
            # rank sees different shapes), so the collective pattern must not depend on that choice — the bucketed
            # hook-issued exchange below belongs to the eager engine only
            fb = self._body_fb(x, y, iteration)
            if self._calib_want:      # the watchdog's eager comparison step: timed up to here, like a probed replay
                self._calib_end = torch.cuda.Event(enable_timing=True)
                self._calib_end.record()
            return self._reduce_and_step(fb)
        import t2v_hip
        opt = self.optimizer
        opt.zero_grad()
        t2v_hip.stamp('step_begin')
        y_pred = self.model(x) if self.allreduce is not None else self._forward(x)
        loss, recon, kl, w = self.criterion(y_pred, y, iteration, lengths=(x[1], x[4]))
        t2v_hip.stamp('loss_end')
        if self.allreduce is not None:
            self.allreduce.begin()
            loss.backward()         # (a multi-rank engine that reaches this line is the eager one: hook-issued buckets)
        else:
            self._backward(loss)
        t2v_hip.stamp('bwd_main_end')
        self.overlap.join()             # weight gradients were produced on the deferred-work stream
        t2v_hip.stamp('grads_ready')
        if self.allreduce is not None:
            # the poison slot is NOT part of a hook-issued bucket (the last bucket leaves during backward, before this
            # step's ledger words exist): finish() reduces the 16-byte tail by itself, after _poison() has written it
            self._poison()
            self.allreduce.finish()
            opt.mark_gathered()        # every bucket gathered its slice before it went out
        opt.guard = self._guard_words()
        grad_norm = opt.step()
        t2v_hip.stamp('step_end')
        return loss.detach(), recon.detach(), kl.detach(), grad_norm

    def _guard_words(self):
        """the error-ledger words this step's cooperative / persistent kernels wrote so far: the fused optimiser step skips the
        update on the device when one of them is set (a spin time-out must not reach the weights).  Multi-rank: the
        guard is the poison slot at the tail of the gradient arena, which _poison() filled before the all-reduce — summed over
        the ranks, so that ALL ranks skip when ONE timed out."""
        import t2v_hip
        if self.allreduce is not None:
            return self.optimizer.poison_slot()[:1].view(torch.int32)
        return self._step_words()

    def _step_words(self):
        """ledger words of THIS step: the block of the graph that was just replayed (a replay runs no host code, so it leaves
        no eager notes — its gather launches rewrite the graph's own block), else the eager notes since the step's mark"""
        import t2v_hip
        if self._err_span is not None:
            return t2v_hip.err_words(self._err_span)
        return t2v_hip.err_range(self._err_mark)

    def _poison(self):
        """multi-rank, before the gradient exchange: poison slot = 1.0 if any of this rank's ledger words of the step is set"""
        words = self._step_words()
        slot = self.optimizer.poison_slot()
        if words is None:
            slot.zero_()
        else:
            slot.copy_(words.ne(0).any().to(torch.float32).expand(4))

    def recover(self, err):
        """Called by the loop when check_async_errors() raised after a step.  If the time-out came from the persistent decoder
        kernels (256 workgroups that need the whole chip to themselves: a GPU shared with another process, a communication
        kernel holding CUs), the device skipped that step's update — weights and Adam moments are intact.  Latch the
        launch-per-step kernels, drop the captured graphs, restore the BatchNorm running statistics (the failed forward pass
        fed them garbage), take the optimiser's step counter back, and tell the caller to run the iteration again.
        The weight average (hparams.ema_decay > 0) needs no repair: it is updated by the very launch that skipped, which
        leaves the shadow untouched like the weights, and the re-run publishes the same iteration, hence the same rate."""
        import t2v_hip
        labels = getattr(err, 'labels', None) or []
        if not labels or not all('persistent kernel' in l for l in labels):
            return False
        print("Warning! persistent decoder kernels could not be co-scheduled (%s); using the launch-per-step kernels from now on"
              % ", ".join(labels))
        t2v_hip.DecoderCore.persistent = False
        t2v_hip.DecoderCore.persistent_bwd = False
        # the watchdog's timings belong to the graphs (and the kernel set) that just went: a re-captured graph on the launch-per-step
        # kernels is probed from scratch, and a shape dropped because it lost against the old eager step gets another chance
        self._cache.clear()
        self._compare_key = None
        if self._bn_snap is not None:
            torch._foreach_copy_(self._bn_bufs, self._bn_snap)
        self.optimizer.step_count = max(0, self.optimizer.step_count - 1)
        self.recoveries += 1
        return True

    def note_good_step(self):
        """the loop calls this after a step whose error check came back clean: one multi-tensor copy keeps a snapshot of the
        BatchNorm running statistics for recover()"""
        if self._bn_snap is None:
            self._bn_bufs = [b for n, b in self.model.named_buffers() if n.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
            self._bn_snap = [b.clone() for b in self._bn_bufs]
        else:
            torch._foreach_copy_(self._bn_snap, self._bn_bufs)

    def step_checked(self, batch, iteration, learning_rate=None):
        """step() + host sync + error check, with ONE automatic re-run on the launch-per-step kernels when the persistent
        decoder kernels timed out (what reference train.py:225-230 does per iteration, loss.item() included)."""
        import t2v_hip
        out = self.step(batch, iteration, learning_rate)
        err = None
        try:
            out[0].item()
            t2v_hip.check_async_errors()
        except t2v_hip.T2VHipError as e:
            err = e
        # every rank reads the same verdict from the device: a skipped step leaves a NaN with a known payload in grad_norm
        # (multi-rank: the poison slot was summed over the ranks, so a time-out on ONE rank skips — and re-runs — the step on ALL)
        skipped = (int(out[4].view(torch.int32).item()) & 0xFFFFFFFF) == self.optimizer.SKIPPED_NORM_BITS
        if err is not None or skipped:
            if err is None:
                err = t2v_hip.T2VHipError("another rank's persistent decoder kernels timed out")
                err.labels = ['decoder (persistent kernel hand-off, remote rank)']
            if not self.recover(err):
                raise err
            out = self.step(batch, iteration, learning_rate)
            out[0].item()
            t2v_hip.check_async_errors()
            # the re-run must have been applied: a second skip (another rank timed out again, a stale poison word) would lose
            # the update silently
            if (int(out[4].view(torch.int32).item()) & 0xFFFFFFFF) == self.optimizer.SKIPPED_NORM_BITS:
                raise t2v_hip.T2VHipError("the re-run of iteration %d on the launch-per-step kernels was skipped as well" % iteration)
        self.note_good_step()
        return out

    def _publish(self, iteration):
        """everything the kernels of this iteration read from the device record, in one upload before the first launch"""
        c = self.criterion
        w = c.kl_weight(iteration)
        sp = self.step_params
        import t2v_hip
        t2v_hip.activate_step_params(sp)
        sp.set(epoch=iteration, kl_weight=w if w is not None else 0.0)
        self.optimizer.publish_step_params(sp)
        sp.upload()
        return w

    def step(self, batch, iteration, learning_rate=None):
        """Body of reference train.py:208-229.  Returns (loss, recon, kl, kl_weight, grad_norm) as
        device tensors / floats without forcing a host sync."""
        if self._stream is not None and torch.cuda.current_stream() != self._stream:
            cur = torch.cuda.current_stream()
            self._stream.wait_stream(cur)
            with torch.cuda.stream(self._stream):
                out = self.step(batch, iteration, learning_rate)
            cur.wait_stream(self._stream)
            return out
        import t2v_hip
        prev = t2v_hip.set_overlap(self.overlap)
        try:
            return self._step(batch, iteration, learning_rate)
        finally:
            t2v_hip.set_overlap(prev)

    def _step(self, batch, iteration, learning_rate):
        import t2v_hip
        self._err_mark = t2v_hip.err_mark()
        self._err_span = None
        self._compare_key = None        # (a comparison request never outlives the step that made it)
        self._calib_end = None
        self._cache.flush_released()    # ledger block of a graph the watchdog dropped during the PREVIOUS step (its words were
                                        # still that step's error record: released only now, after the caller's check)
        if self._bn_snap is None:
            self.note_good_step()       # BatchNorm statistics as loaded (checkpoint / warm start included): what a time-out on
                                        # the very first step restores
        opt = self.optimizer
        if learning_rate is not None:
            opt.param_groups[0]['lr'] = learning_rate
        w = self._publish(iteration)
        graphable = self.use_graph and self.model.training
        out = None
        if not any(t.is_cuda for t in batch):
            # host batch: one pinned staging buffer, one H2D copy — straight into the static input buffer of the
            # captured graph when this shape has one
            lay = BatchLayout(batch)
            if graphable:
                def make_static():
                    buf = torch.empty(lay.nbytes, dtype=torch.uint8, device='cuda')
                    lay.upload(batch, into=buf)
                    return lay.views(buf) + ([buf],)
                out = self._graph_step(('staged',) + lay.key, make_static, lambda static: lay.upload(batch, into=static[0]), iteration)
            if out is None:
                x, y = lay.views(lay.upload(batch))
        else:           # the device front end already produced device tensors
            x, y = self.model.parse_batch(batch)
            if graphable:
                tensors = [t for t in x if torch.is_tensor(t)] + list(y)

                def make_static():
                    static_x = tuple(t.clone() if torch.is_tensor(t) else t for t in x)
                    static_y = tuple(t.clone() for t in y)
                    return static_x, static_y, [t for t in static_x if torch.is_tensor(t)] + list(static_y)

                def load(static):
                    for dst, src in zip(static, tensors):
                        if dst.data_ptr() != src.data_ptr():
                            dst.copy_(src, non_blocking=True)
                key = tuple((tuple(t.shape), str(t.dtype)) for t in tensors) + (int(x[3]),)
                out = self._graph_step(key, make_static, load, iteration)
        if out is not None:
            return out[0], out[1], out[2], w, out[3]
        # Eager steps: keep the host at most two steps ahead of the GPU (it issues a step in ~5.5 ms, the GPU needs 13.5): a
        # caller that never reads a result back (the reference loop does, train.py:230 `loss.item()`) would otherwise run
        # hundreds of steps ahead until the hardware queue is full.
        ring = self._eager_events
        if len(ring) >= 2:
            ring.pop(0).synchronize()
        key, self._compare_key = self._compare_key, None
        t0 = None
        if key is not None:      # the watchdog's eager comparison step of a freshly captured shape (graph_cache.py)
            t0 = torch.cuda.Event(enable_timing=True)
            t0.record()
        self._calib_want = t0 is not None
        loss, recon, kl, grad_norm = self._body(x, y, iteration)
        self._calib_want = False
        ev = torch.cuda.Event(enable_timing=t0 is not None)
        ev.record()
        if t0 is not None:
            self._cache.compared(key, t0, self._calib_end or ev)
        ring.append(ev)
        return loss, recon, kl, w, grad_norm

    # -- graph path
    def _graph_step(self, key, make_static, load, iteration):
        """One sight of the shape `key`: the step's results when it ran as a graph, None when it has to run eagerly (a shape that is
        still warming up, the watchdog's comparison step, a dropped graph, no ledger block free for the capture).
        make_static() -> (x, y, static inputs) holding this batch, for a capture; load(static inputs) brings this batch into the
        static inputs of a graph that exists."""
        what, entry = self._cache.sight(key)
        if what == CAPTURE:
            static_x, static_y, static = make_static()
            cap = self._capture_static(static_x, static_y, iteration)
            if cap is None:
                return None
            self._cache.store(key, cap[0], static, *cap[1:])
        elif what == REPLAY:
            load(entry.static)
        else:
            if what == COMPARE:
                self._compare_key = key
            return None
        return self._cache.replay(key, self._after_replay, self._replay_drag if self._test_replay_drag_us else None)

    def _replay_drag(self):
        import t2v_hip
        t2v_hip.load_library().t2v_debug_spin(8, int(self._test_replay_drag_us), t2v_hip._stream())

    def _after_replay(self, entry):
        """the captured graph writes its scalars (loss, recon, kl[, grad_norm]) into static tensors that the NEXT replay
        overwrites: hand the caller fresh copies (one small launch), like the eager path does"""
        vals = torch.cat([t.reshape(1) for t in entry.out])
        base = 3 if self.graph_ddp else 4
        if len(entry.out) > base:         # a graph with the KL control launch: the criterion shows THIS step's K', T and floored count
            self.criterion.kl_floored_sum, self.criterion.kl_objective, self.criterion.kl_floored_dims = vals[base:base + 3].unbind()
        self._err_span = entry.span       # the words this replay wrote: what _poison() / the optimiser guard read
        if self._test_after_replay is not None:     # (tests: a time-out inside a REPLAY — no host code runs there that could be intercepted)
            self._test_after_replay(entry.span)
        if self.graph_ddp:
            return self._reduce_and_step((vals[0], vals[1], vals[2]), entry.no_grad)
        self.optimizer.step_count += 1
        return vals[0], vals[1], vals[2], vals[3:4]

    def _capture_static(self, static_x, static_y, iteration):
        import t2v_hip
        # the ledger words of the captured launches live in a block of their own, rewritten by every replay and released when
        # the graph is evicted; with no block free the shape simply keeps running eagerly
        if not t2v_hip.err_capture_begin():
            return None
        torch.cuda.synchronize()
        count0 = self.optimizer.step_count
        dot = os.environ.get('T2V_GRAPH_DOT')       # measurement (tools/graph_critical_path.py): the captured DAG as a DOT file
        graph = torch.cuda.CUDAGraph(keep_graph=True) if dot else torch.cuda.CUDAGraph()
        # with a process group alive its watchdog thread polls events while this thread captures: under the default
        # 'global' error mode such a query from ANOTHER thread aborts the process now and then (seen as exit code -6 in
        # one of five runs); 'thread_local' restricts the check to this thread — the launches of the autograd worker
        # thread are still captured (capture follows the stream, not the thread)
        mode = 'thread_local' if self.allreduce is not None else 'global'
        span = None
        try:
            self._err_mark = t2v_hip.err_mark()     # (inside the block: the captured optimiser guard reads these words)
            with torch.cuda.graph(graph, stream=self._stream, capture_error_mode=mode):
                out = (self._body_fb if self.graph_ddp else self._body)(static_x, static_y, iteration)
            span = t2v_hip.err_capture_end()
            if dot:
                import ctypes
                hip = ctypes.CDLL('libamdhip64.so')
                rc = hip.hipGraphDebugDotPrint(ctypes.c_void_p(graph.raw_cuda_graph()), dot.encode(), ctypes.c_uint(1))
                print("hipGraphDebugDotPrint -> %d (%s)" % (rc, dot), flush=True)
        finally:
            if span is None:
                t2v_hip.err_capture_end(keep=False)
        self.optimizer.step_count = count0      # capture executes nothing; the replay below is this iteration's step
        no_grad = list(self.optimizer._no_grad) if self.graph_ddp else None
        out = tuple(out)
        if self.kl_monitor is not None:     # the KL control launch was captured: its K', T and floored count travel with the step's scalars
            c = self.criterion
            out += (c.kl_floored_sum, c.kl_objective, c.kl_floored_dims)
        return graph, out, no_grad, span


def prepare_directories_and_logger(output_directory, log_directory, rank):
    """reference train.py:68-77: rank 0 owns the output directory and the TensorBoard stream."""
    if rank != 0:
        return None
    if output_directory and not os.path.isdir(output_directory):
        os.makedirs(output_directory)
        os.chmod(output_directory, 0o775)
    if not log_directory:
        return None
    from logger import Tacotron2Logger
    return Tacotron2Logger(os.path.join(output_directory or '.', log_directory))


def prepare_dataloaders(hparams, resident_corpus=False):
    """reference train.py:52-65 (DistributedSampler shards, drop_last, the reference's collate layout).
    Switches the reference does not have, all off by default:
      resident_corpus=True : (an argument, not a hyper-parameter) the training and the validation list are turned into mels
                             once and kept on the GPU (corpus.ResidentCorpus, every rank holds the whole store); trainset and
                             valset are its two views, whose items are utterance indices, and corpus.ResidentCollate
                             assembles a batch with one launch.  Samplers and bucketing are the code below, unchanged;
      device_frontend=True : the dataset returns raw int16 audio, the collate pads it, and the whole batch goes
                             through ONE STFT->mel launch on the GPU (data_utils.DeviceFrontendCollate);
      bucket_batches=True  : batches are drawn from length buckets (data_utils.BucketBatchSampler), so that a
                             batch wastes few padded frames and DP ranks see similar amounts of work."""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    from data_utils import BucketBatchSampler, DeviceFrontendCollate, TextMelCollate, TextMelLoader
    device_fe = bool(getattr(hparams, 'device_frontend', False))
    if device_fe and getattr(hparams, 'load_mel_from_disk', False):
        raise ValueError("device_frontend=True needs raw audio: it cannot be combined with load_mel_from_disk=True "
                         "(the collate would run the STFT over stored mels)")
    if resident_corpus:
        if getattr(hparams, 'load_mel_from_disk', False):
            raise ValueError("resident_corpus=True needs raw audio: it cannot be combined with load_mel_from_disk=True "
                             "(the store is built by the device front end from the wavs)")
        from corpus import ResidentCollate, ResidentCorpus
        corpus = ResidentCorpus([hparams.training_files, hparams.validation_files], hparams)
        if not hparams.distributed_run or dist.get_rank() == 0:
            print(corpus.describe(), flush=True)
        trainset, valset = corpus.view(0), corpus.view(1)
        collate_fn = ResidentCollate(corpus, hparams)
    else:
        trainset = TextMelLoader(hparams.training_files, hparams, return_audio=device_fe)
        valset = TextMelLoader(hparams.validation_files, hparams, return_audio=device_fe)
        collate_fn = (DeviceFrontendCollate(hparams, stft=trainset.stft) if device_fe
                      else TextMelCollate(hparams.n_frames_per_step))
    if getattr(hparams, 'bucket_batches', False):
        world, rank = (dist.get_world_size(), dist.get_rank()) if hparams.distributed_run else (1, 0)
        batch_sampler = BucketBatchSampler(trainset.lengths(), hparams.batch_size, world_size=world, rank=rank,
                                           seed=hparams.seed, text_lengths=trainset.text_lengths())
        loader = DataLoader(trainset, num_workers=0, batch_sampler=batch_sampler, pin_memory=False,
                            collate_fn=collate_fn)
    else:
        sampler = DistributedSampler(trainset) if hparams.distributed_run else None
        loader = DataLoader(trainset, num_workers=0, shuffle=False, sampler=sampler, batch_size=hparams.batch_size,
                            pin_memory=False, drop_last=True, collate_fn=collate_fn)
    return loader, valset, collate_fn


def validate(model, criterion, valset, iteration, batch_size, n_gpus, collate_fn, logger, distributed_run, rank, ema=False,
             kl_active_units=None):
    """reference train.py:122-147, including its habit of reporting the LAST batch's loss (B-13).  ema=True: the caller has
    put the averaged weights into the model (FlatAdam.swapped_ema); the loss is printed and logged under its own name and
    the histograms / images of log_validation are not written a second time.  kl_active_units: what the KL monitor counted over
    the training batches since the last validation (a run that keeps one), logged beside the validation loss."""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    model.eval()
    reduced = float('nan')
    y = y_pred = None
    with torch.no_grad():
        sampler = DistributedSampler(valset) if distributed_run else None
        loader = DataLoader(valset, sampler=sampler, num_workers=0, shuffle=False, batch_size=batch_size,
                            pin_memory=False, collate_fn=collate_fn)
        for batch in loader:
            x, y = model.parse_batch(batch)
            y_pred = model(x)
            # (the lengths go along as in a training step; under no_grad the criterion leaves the guided attention term out:
            # validation.loss stays the reference's)
            loss, _, _, _ = criterion(y_pred, y, iteration, lengths=(x[1], x[4]))
            reduced = (t2v_dist.reduce_tensor(loss.data, n_gpus) if distributed_run else loss).item()
    model.train()
    t2v_hip_check()
    if rank == 0 and ema:
        print("Validation loss (ema) {}: {:9f}  ".format(iteration, reduced))
        if logger is not None and y_pred is not None:
            logger.log_validation_ema(reduced, iteration)
    elif rank == 0:
        print("Validation loss {}: {:9f}  ".format(iteration, reduced))
        if logger is not None and y_pred is not None:
            if kl_active_units is None:
                logger.log_validation(reduced, model, y, y_pred, iteration)
            else:
                logger.log_validation(reduced, model, y, y_pred, iteration, kl_active_units=kl_active_units)
    return reduced


def train(output_directory, log_directory, checkpoint_path, warm_start, n_gpus, rank, group_name, hparams,
          resident_corpus=False):
    if hparams.distributed_run:
        t2v_dist.init_distributed(hparams, n_gpus, rank, group_name)
        n_gpus, rank = dist.get_world_size(), dist.get_rank()
    torch.manual_seed(hparams.seed)
    torch.cuda.manual_seed(hparams.seed)
    engine = TrainEngine(hparams, world_size=n_gpus if hparams.distributed_run else 1)
    model, optimizer, criterion = engine.model, engine.optimizer, engine.criterion
    learning_rate = hparams.learning_rate
    logger = prepare_directories_and_logger(output_directory, log_directory, rank)
    train_loader, valset, collate_fn = prepare_dataloaders(hparams, resident_corpus=resident_corpus)

    iteration, epoch_offset = 0, 0
    if checkpoint_path is not None:
        if warm_start:
            warm_start_model(checkpoint_path, model, optimizer)
        else:
            _, _, saved_lr, iteration = load_checkpoint(checkpoint_path, model, optimizer)
            if hparams.use_saved_learning_rate:
                learning_rate = saved_lr
            iteration += 1
            epoch_offset = max(0, int(iteration / len(train_loader)))

    # the whole loop runs on the engine's stream (graph_step, the default): a step then needs no hand-over with the
    # caller's stream (≈1.7 ms per step otherwise) and `python train.py` delivers what bench.py measures
    with engine.stream_context():
        for epoch in range(epoch_offset, hparams.epochs):
            print("Epoch: {}".format(epoch))
            if hasattr(getattr(train_loader, 'batch_sampler', None), 'set_epoch'):
                train_loader.batch_sampler.set_epoch(epoch)
                hit = train_loader.batch_sampler.persistent_hit_rate()
                if hit is not None and rank == 0:
                    print("Batches inside the persistent decoder kernels' range (T_in <= {}): {:.1f} %".format(
                        train_loader.batch_sampler.text_cap, 100.0 * hit))
            for batch in train_loader:
                start = time.perf_counter()
                # (syncs and checks the error ledger like the .item() of reference train.py:230; a time-out of the persistent
                # decoder kernels re-runs the iteration once on the launch-per-step kernels)
                loss, recon, kl, kl_w, grad_norm = engine.step_checked(batch, iteration, learning_rate)
                reduced = (t2v_dist.reduce_tensor(loss, n_gpus) if hparams.distributed_run else loss).item()
                if not math.isnan(reduced) and rank == 0:
                    duration = time.perf_counter() - start
                    guided = criterion.guided.item() if hparams.guided_attention_weight > 0 else None
                    # free bits / capacity: the KL objective T (training.loss carries w * T; kl_div stays the raw KL) and the
                    # number of floored dimensions of this step
                    klc = ({'kl_objective': criterion.kl_objective.item(), 'kl_floored_dims': int(criterion.kl_floored_dims.item())}
                           if criterion.kl_control else {})
                    print("Train loss {} {:.6f} Grad Norm {:.6f} {:.2f}s/it".format(
                        iteration, reduced, grad_norm.item(), duration) +
                        ("" if guided is None else " Guided attention {:.6f}".format(guided)) +
                        ("" if not klc else " KL objective {kl_objective:.6f} floored dims {kl_floored_dims}".format(**klc)))
                    if logger is not None:
                        logger.log_training(reduced, grad_norm.item(), learning_rate, duration, recon.item(), kl.item(),
                                            kl_w, iteration, guided_attention=guided, **klc)
                if iteration % hparams.iters_per_checkpoint == 0:
                    active = None
                    if engine.kl_monitor is not None:
                        # the window since the last validation (this rank's training batches), read where the loop synchronises anyway
                        seen = engine.kl_monitor.read()
                        engine.kl_monitor.reset()
                        active = seen['active_units']
                        if rank == 0:
                            print("KL monitor {}: active units {} of {} over {} utterances".format(
                                iteration, active, engine.kl_monitor.dims, seen['n']))
                    validate(model, criterion, valset, iteration, hparams.batch_size, n_gpus, collate_fn, logger,
                             hparams.distributed_run, rank, kl_active_units=active)
                    if optimizer.ema is not None:
                        with optimizer.swapped_ema():
                            validate(model, criterion, valset, iteration, hparams.batch_size, n_gpus, collate_fn, logger,
                                     hparams.distributed_run, rank, ema=True)
                    if rank == 0:
                        save_checkpoint(model, optimizer, learning_rate, iteration,
                                        os.path.join(output_directory, "checkpoint_{}".format(iteration)))
                iteration += 1
    if logger is not None:
        logger.close()


def cli_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('-o', '--output_directory', type=str, help='directory to save checkpoints')
    ap.add_argument('-l', '--log_directory', type=str, help='directory to save tensorboard logs')
    ap.add_argument('-c', '--checkpoint_path', type=str, default=None, required=False, help='checkpoint path')
    ap.add_argument('--warm_start', action='store_true', help='load the model only (warm start)')
    ap.add_argument('--n_gpus', type=int, default=1, required=False, help='number of gpus')
    ap.add_argument('--rank', type=int, default=0, required=False, help='rank of current gpu')
    ap.add_argument('--group_name', type=str, default='group_name', required=False, help='Distributed group name')
    ap.add_argument('--hparams', type=str, required=False, help='comma separated name=value pairs')
    ap.add_argument('--resident_corpus', action='store_true',
                    help='keep the training and validation sets on the GPU as mels and collate every batch with one kernel')
    return ap


if __name__ == '__main__':
    args = cli_parser().parse_args()
    hp = create_hparams(args.hparams)
    print("Distributed Run:", hp.distributed_run)
    train(args.output_directory, args.log_directory, args.checkpoint_path, args.warm_start, args.n_gpus,
          args.rank, args.group_name, hp, resident_corpus=args.resident_corpus)
