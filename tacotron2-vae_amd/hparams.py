"""Plain-Python hyper-parameter bag for the MI355X Tacotron2-VAE path.

Mirrors the attribute names/defaults of the reference's TF1 `HParams` object
(reference hparams.py:6-117) and its "k=v,k=v" override string
(hparams.py:119-121), without the tensorflow dependency.
"""

_GROUPS = {
    'experiment': dict(
        epochs=300, iters_per_checkpoint=500, seed=1234, dynamic_loss_scaling=True,
        fp16_run=False, distributed_run=False, dist_backend="nccl",
        dist_url="tcp://localhost:54321", cudnn_enabled=True, cudnn_benchmark=True),
    'data': dict(
        load_mel_from_disk=False, training_files='filelists/ms_kor_train.txt',
        validation_files='filelists/ms_kor_val.txt', text_cleaners=['korean_cleaners'],
        sort_by_length=False),
    'audio': dict(
        max_wav_value=32768.0, sampling_rate=16000, filter_length=1024, hop_length=256,
        win_length=1024, n_mel_channels=80, mel_fmin=0.0, mel_fmax=8000.0),
    'text_encoder': dict(
        n_symbols=80, symbols_embedding_dim=512, encoder_kernel_size=5,
        encoder_n_convolutions=3, encoder_embedding_dim=512),
    'labels': dict(n_speakers=1, speaker_embedding_dim=16, n_emotions=4,
                   emotion_embedding_dim=16),
    'vae': dict(
        E=512, ref_enc_filters=[32, 32, 64, 64, 128, 128], ref_enc_size=[3, 3],
        ref_enc_strides=[2, 2], ref_enc_pad=[1, 1], ref_enc_gru_size=256,
        z_latent_dim=32, anneal_function='logistic', anneal_k=0.0025, anneal_x0=10000,
        anneal_upper=0.2, anneal_lag=50000),
    'prosody_unused': dict(
        prosody_n_convolutions=6, prosody_conv_dim_in=[1, 32, 32, 64, 64, 128],
        prosody_conv_dim_out=[32, 32, 64, 64, 128, 128], prosody_conv_kernel=3,
        prosody_conv_stride=2, prosody_embedding_dim=128),
    'decoder': dict(
        n_frames_per_step=1, decoder_rnn_dim=1024, prenet_dim=256, max_decoder_steps=1000,
        gate_threshold=0.5, p_attention_dropout=0.1, p_decoder_dropout=0.1,
        attention_rnn_dim=1024, attention_dim=128, attention_location_n_filters=32,
        attention_location_kernel_size=31),
    'postnet': dict(postnet_embedding_dim=512, postnet_kernel_size=5,
                    postnet_n_convolutions=5),
    'optim': dict(use_saved_learning_rate=False, learning_rate=1e-3, weight_decay=1e-6,
                  grad_clip_thresh=1.0, batch_size=64, mask_padding=True),
}


# Switches this build adds (not in the reference's HParams; `values()` keeps reporting the reference's set only):
#   device_frontend : dataset hands over raw int16 audio, ONE batched STFT->mel launch per batch on the GPU
#   bucket_batches  : length-bucketed batch sampler (low padding waste, balanced DP ranks)
#   bf16_run        : bf16 MFMA for the Postnet/encoder convolutions and the time-batched linears, fp32
#                     master weights / accumulation / BatchNorm / recurrent state (replaces fp16_run)
#   graph_step      : capture the whole training iteration into a HIP graph per input shape and replay it
#                     (train.TrainEngine).  ON by default: a shape is captured the third time it is seen (at most 8
#                     shapes), so fixed / bucketed shapes replay and ragged batches whose shapes never repeat simply
#                     stay eager; `python train.py` then runs what bench.py measures
#   fp32_allreduce  : True (default, like the reference: distributed.py reduces fp32): the gradient exchange stays fp32 under
#                     bf16_run as well (115.5 MB per step); False opts in to the bf16 wire format (57.7 MB; every slice is
#                     rounded to bf16 and summed over the ranks in bf16: relative error ~ sqrt(world) * 2^-9 per element)
_EXTENSIONS = dict(device_frontend=False, bucket_batches=False, bf16_run=False, graph_step=True, fp32_allreduce=True)

# The training recipe's own switches: what the loop does with the weights, not how the build runs a step.  A third group,
# reported by `recipe()` alone (`values()` stays the reference's set, `extensions()` the build's):
#   ema_decay  : 0 (default) = off.  Otherwise an exponential moving average of the weights is kept beside Adam, in the
#                same fused launch (optim.FlatAdam), saved in the checkpoint as 'ema_state_dict' and validated next to the
#                raw weights; `--weights ema` of synthesizer.py / evaluate.py / extract_latents.py reads it.  0.9999 is the
#                usual choice for Tacotron-like models
#   ema_warmup : the decay of update t is min(ema_decay, (1 + t) / (10 + t)), so that the average does not sit on the
#                initial weights for the first 1 / (1 - ema_decay) iterations
#   guided_attention_weight : 0 (default) = off.  Otherwise weight x the guided attention loss (Tachibana et al.; ESPnet's
#                GuidedAttentionLoss) is added to the TRAINING loss: a penalty on attention weight far from the diagonal, which
#                helps the decoder find a monotonic alignment early.  1.0 is the usual choice.  A training aid, not a model
#                score: the validation loss stays the reference's (the term is left out there), so that validation.loss is
#                comparable between runs with and without it.  Constant over a run (no schedule)
#   guided_attention_sigma  : width of the diagonal band the penalty leaves free (ESPnet's default 0.4)
#   kl_free_bits : 0 (default) = off.  Otherwise lambda, in nats per latent dimension (free bits, Kingma et al. 2016, in the
#                batch-mean form): the KL term of the TRAINING loss becomes K' = B * sum_d max(k[d], lambda), k[d] the batch mean
#                of the KL of dimension d.  A dimension at or under lambda is floored: it costs the constant B * lambda and gets no
#                KL gradient, so the optimiser gains nothing by emptying it further
#   kl_capacity  : negative (default) = off.  Otherwise C, in nats per utterance (Burgess et al. 2018; Battenberg et al. 2019
#                for expressive Tacotron): the KL term becomes |K' - B * C|, which pulls the KL TOWARDS C instead of towards 0.
#                Constant over a run (no schedule), frozen in a captured step like guided_attention_weight
#   anneal_cycle, anneal_ratio : anneal_function=cyclical (Fu et al. 2019): the KL weight ramps from 0 to anneal_upper over the first
#                anneal_ratio of every anneal_cycle steps and stays there for the rest of the cycle
#   kl_monitor   : True keeps a running per-dimension record of the posterior inside the loss launch (t2v_hip.KLMonitor): the loop
#                prints and logs the active units of the window at every validation.  A free-bits or capacity run keeps one anyway
# Like the guided attention term these shape the training loss only: validation.loss and the logged kl_div stay the reference's.
_RECIPE = dict(ema_decay=0.0, ema_warmup=True, guided_attention_weight=0.0, guided_attention_sigma=0.4)
# (the VAE half of the group, kept under a name of its own: tests/test_guided_host.py pins the keys of _RECIPE)
_RECIPE_VAE = dict(kl_free_bits=0.0, kl_capacity=-1.0, anneal_cycle=10000, anneal_ratio=0.5, kl_monitor=False)
_RECIPE_ALL = dict(_RECIPE, **_RECIPE_VAE)      # the recipe group: what recipe() reports and values() leaves out
# Switches of the group that an hparams object stores only once they are set: left alone, they read as their defaults above and
# appear in no listing, so `recipe()`, the store and whatever is printed or saved from them are, for a run that does not use
# such a switch, what they were before the switch existed.
_RECIPE_UNSTORED = ('guided_attention_weight', 'guided_attention_sigma') + tuple(_RECIPE_VAE)


def _coerce(old, text):
    if isinstance(old, bool):
        return text.strip().lower() in ('true', '1')
    if isinstance(old, int):
        return int(text)
    if isinstance(old, float):
        return float(text)
    if isinstance(old, (list, tuple)):
        raise ValueError("list-valued hparams cannot be overridden from a string")
    return text


class HParams(object):
    """Attribute bag with `.parse("a=1,b=x")` and `.values()`."""

    def __init__(self, **kw):
        object.__setattr__(self, '_store', {})
        for k, v in kw.items():
            self._store[k] = v

    def __getattr__(self, k):
        store = object.__getattribute__(self, '_store')
        if k in store:
            return store[k]
        if k in _RECIPE_UNSTORED:
            return _RECIPE_ALL[k]
        raise AttributeError(k)

    def __setattr__(self, k, v):
        self._store[k] = v

    def __contains__(self, k):
        return k in self._store

    def values(self):
        """the reference's hyper-parameters (build-specific switches excluded)"""
        return {k: v for k, v in self._store.items() if k not in _EXTENSIONS and k not in _RECIPE_ALL}

    def extensions(self):
        return {k: v for k, v in self._store.items() if k in _EXTENSIONS}

    def recipe(self):
        return {k: v for k, v in self._store.items() if k in _RECIPE_ALL}

    def parse(self, spec):
        for item in filter(None, (s.strip() for s in spec.split(','))):
            if '=' not in item:
                raise ValueError("bad hparams item %r (want name=value)" % item)
            k, v = (s.strip() for s in item.split('=', 1))
            if k not in self._store and k not in _RECIPE_UNSTORED:
                raise ValueError("unknown hparam %r" % k)
            self._store[k] = _coerce(getattr(self, k), v)
        return self


def create_hparams(hparams_string=None, verbose=False):
    """Same call signature as reference hparams.py:3."""
    flat = {}
    for grp in _GROUPS.values():
        for k, v in grp.items():
            flat[k] = list(v) if isinstance(v, list) else v
    flat.update(_EXTENSIONS)
    flat.update({k: v for k, v in _RECIPE.items() if k not in _RECIPE_UNSTORED})
    hp = HParams(**flat)
    if hparams_string:
        hp.parse(hparams_string)
    if verbose:
        print('hparams:', hp.values())
    return hp
