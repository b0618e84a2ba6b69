"""Reference of the STFT -> mel front end (csrc/frontend.hip: k_mel_frontend) — TEST INFRASTRUCTURE, NOT PRODUCT.

  mel()      reflect pad 512 (edge sample excluded), frames at hop 256, periodic Hann, rfft, magnitude, bank @ magnitude, in the
             dtype asked for (float64: the reference; float32: the same operation at the kernel's precision).  It returns the
             LINEAR mel: the logarithm is undone on the device's side (compare()), because bands far from a tone sit on the fp32
             leakage floor (~1e-9 of the peak) and a logarithm turns that round-off into any relative error one likes.
  The bank is the one the module under test built (TacotronSTFT.mel_basis, fp32 values), in both dtypes: the filterbank
  formula is tested elsewhere (tests/test_oracle_golden.py), this reference tests the transform.

The metric.  fp32 round-off of an FFT followed by a non-negative weighted sum scales with
      scale[m, t] = sum_k w[m, k] * (|X64[k, t]| + ||frame_t * window||_2)
(the first term dominates on tones, the second on noise: an FFT's error in one bin is relative to the frame's norm, not to the
bin).  floor = max |mel32 - mel64| / scale over a case, computed on the host of the same run.  An entry passes below
      bound[m, t] = K * max(floor, 4 * 2^-24) * scale[m, t] + 2^-19 * max(mel64[m, t], 1e-5),   K = 16
(the rule of tests/test_recurrent_edges_gpu.py; the last term is two ulps of an fp32 logarithm of magnitude below 16, which is
what turning the kernel's log output back into a linear value costs).  compare() measures |exp(out_log) - max(mel64, 1e-5)|
entry by entry; the clamp is 1-Lipschitz, so no entry is left out, neither near the clamp nor in clamped bands.

A `mutation` is a one-line wrong variant that models a kernel slip; tests/test_frontend_ref.py shows on the reference alone
that each stands at least 100 bounds above the reference on its designated signal.
"""
import collections
import math

import torch

N_FFT, HOP, N_MEL, N_BINS = 1024, 256, 80, 513
CLAMP = 1e-5
ULP4 = 4.0 * 2.0 ** -24
LOG_ULPS = 2.0 ** -19

MUTATIONS = ('edge', 'shift', 'symhann', 'mirror', 'tap_last', 'tap_first', 'tap21', 'tap41')

# (sampling rate, fmin, fmax, registers path?)  The last column is what registers_path() must say: a filter of lanes 0..63
# wider than 20 taps, or one of 64..79 wider than 40, sends the kernel to its CSR loop.
BANKS = ((16000, 0.0, 8000.0, True), (22050, 0.0, 8000.0, True), (16000, 80.0, 7600.0, True), (48000, 0.0, 8000.0, True),
         (22050, 0.0, 11025.0, False), (24000, 0.0, 12000.0, False), (44100, 0.0, 22050.0, False))
DEFAULT_BANK = BANKS[0]
FALLBACK_BANK = BANKS[4]

Ref = collections.namedtuple('Ref', 'mel mag norm')


def bank_name(bank):
    return '%d/%g/%g' % bank[:3]


def registers_path(stft):
    """True when k_mel_frontend takes its LDS-tap mel loop for this filterbank, False when it takes the CSR loop: the
    kernel's own predicate `mel_regs`, on the host tables.  20 is FE_W1 and 40 is 4 * FE_W2Q of csrc/frontend.hip."""
    ln = stft._host_tables['mel_len']
    return bool(ln[:64].max() <= 20 and ln[64:].max() <= 40)


# ------------------------------------------------------------------------------------------------ signals
def _gen(name, seed):
    return torch.Generator().manual_seed(1000003 * seed + sum(ord(ch) for ch in name))


def signal(name, n, seed=0, k0=0):
    """n seeded samples in [-1, 1], float32.  k0: the first bin of 'steptone' (segment j sits on bin 1 + (k0 + j) % 511) and
    the bin of 'tone'."""
    g = _gen(name, seed)
    i = torch.arange(n, dtype=torch.float64)
    if name == 'noise':
        x = torch.clamp(0.1 * torch.randn(n, generator=g, dtype=torch.float64), -1, 1)
    elif name == 'faint':                                   # straddles the 1e-5 clamp
        x = 1e-4 * torch.randn(n, generator=g, dtype=torch.float64)
    elif name == 'steptone':                                # 1024-sample segments, each on the next integer bin
        seg = (i // N_FFT).long()
        nseg = int(seg.max()) + 1 if n else 0
        phi = 2 * math.pi * torch.rand(nseg, generator=g, dtype=torch.float64)
        k = (1 + (k0 + seg) % 511).double()
        x = 0.5 * torch.cos(2 * math.pi * k * i / N_FFT + phi[seg])
    elif name == 'tone':                                    # one integer bin, for the single-tap mutations
        phi = 2 * math.pi * torch.rand(1, generator=g, dtype=torch.float64)
        x = 0.5 * torch.cos(2 * math.pi * k0 * i / N_FFT + phi)
    elif name == 'halfbin':                                 # halfway between two bins: the worst leakage there is
        phi = 2 * math.pi * torch.rand(2, generator=g, dtype=torch.float64)
        x = 0.45 * torch.cos(2 * math.pi * 37.5 * i / N_FFT + phi[0]) + 0.45 * torch.cos(2 * math.pi * 511.5 * i / N_FFT + phi[1])
    elif name == 'clicks':                                  # where the reflection and the first / last two frames differ
        x = torch.zeros(n, dtype=torch.float64)
        for j, p in enumerate((1, 511, 512, n - 513, n - 2)):
            x[p] = 0.9 if j % 2 == 0 else -0.9
    elif name == 'square':                                  # exactly +-1
        x = torch.where((i.long() // 19) % 2 == 0, 1.0, -1.0).double()
    elif name == 'silence':
        x = torch.zeros(n, dtype=torch.float64)
    else:
        raise KeyError(name)
    x = x.float()
    assert x.numel() == 0 or (float(x.min()) >= -1 and float(x.max()) <= 1)
    return x


def batch(name, lens, N=None, k0_step=0):
    """(B, N) float32, row b = signal(name, lens[b], seed b) and zeros behind it (N: the longest row when None)"""
    N = max(lens) if N is None else N
    wav = torch.zeros(len(lens), N)
    for b, n in enumerate(lens):
        wav[b, :n] = signal(name, n, seed=b, k0=k0_step * b)
    return wav


# ------------------------------------------------------------------------------------------------ the reference
def tap_bin(bank, mutation):
    """(filter, bin) of the tap a tap mutation drops, in the (80, 513) bank"""
    nz = [torch.nonzero(row).flatten() for row in bank]
    if mutation == 'tap_last':
        return 40, int(nz[40][-1])
    if mutation == 'tap_first':
        return 70, int(nz[70][0])
    lo, hi, tap = (0, 64, 20) if mutation == 'tap21' else (64, 80, 40)
    for m in range(lo, hi):
        if len(nz[m]) and int(nz[m][-1] - nz[m][0]) >= tap:        # the filter has a tap of that index
            return m, int(nz[m][0]) + tap
    raise ValueError("%s: no filter of %d..%d has a tap %d in this bank" % (mutation, lo, hi - 1, tap))


def window(dtype, mutation=None):
    i = torch.arange(N_FFT, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2 * math.pi * i / (N_FFT - 1 if mutation == 'symhann' else N_FFT))).to(dtype)


def frames(y, n, dtype, mutation=None):
    """(T, 1024) windowed frames of y[:n], T = n // 256 + 1"""
    assert n > N_FFT // 2, n
    x = y[:n].to(dtype)
    T = n // HOP + 1
    p = torch.arange(-(N_FFT // 2), n + N_FFT // 2 + 1)
    if mutation == 'edge':                                  # the reflection includes the edge sample
        p = torch.where(p < 0, -p - 1, p)
        p = torch.where(p >= n, 2 * n - 1 - p, p)
    else:
        p = torch.where(p < 0, -p, p)
        p = torch.where(p >= n, 2 * (n - 1) - p, p)
    padded = x[p.clamp(0, n - 1)]
    if mutation == 'shift':                                 # frames one sample late
        padded = padded[1:]
    return padded.unfold(0, N_FFT, HOP)[:T] * window(dtype, mutation)


def mel(y, n, bank, dtype, mutation=None):
    """Ref(linear mel (80, T), magnitudes (513, T), ||frame * window||_2 (T)) of y[:n] in `dtype`"""
    assert mutation is None or mutation in MUTATIONS, mutation
    assert dtype in (torch.float64, torch.float32)
    xw = frames(y, n, dtype, mutation)
    mag = torch.fft.rfft(xw, dim=1).abs().t().contiguous()
    if mutation == 'mirror':                                # the untangle's k and 512 - k
        mag[[100, 412]] = mag[[412, 100]]
    w = bank.to(dtype)
    if mutation in ('tap_last', 'tap_first', 'tap21', 'tap41'):
        w = w.clone()
        w[tap_bin(bank, mutation)] = 0
    return Ref(w @ mag, mag, xw.norm(dim=1))


def scale(bank, ref64):
    """what the fp32 round-off of this entry scales with, (80, T)"""
    return bank.double() @ (ref64.mag + ref64.norm[None, :])


def floor(refs32, refs64, bank):
    """max |mel32 - mel64| / scale over the rows of a case (an entry of scale 0 has mel32 = mel64 = 0)"""
    f = 0.0
    for r32, r64 in zip(refs32, refs64):
        s = scale(bank, r64)
        d = (r32.mel.double() - r64.mel).abs()
        assert bool((d[s == 0] == 0).all())
        f = max(f, float((d / s.clamp(min=1e-300)).max()))
    return f


def bound(bank, ref64, flr, K=16.0):
    return K * max(flr, ULP4) * scale(bank, ref64) + LOG_ULPS * ref64.mel.clamp(min=CLAMP)


def compare(out_log, mel64, bnd):
    """the kernel's (or anyone's) LOG mel (80, T) against a linear fp64 mel, entry by entry, no entry left out:
    (largest err / bound, its err, its bound, its (m, t))"""
    assert out_log.shape == mel64.shape == bnd.shape, (out_log.shape, mel64.shape, bnd.shape)
    assert bool(torch.isfinite(out_log).all())
    err = (torch.exp(out_log.double()) - mel64.clamp(min=CLAMP)).abs()
    ratio = err / bnd
    i = int(ratio.argmax())
    m, t = i // ratio.shape[1], i % ratio.shape[1]
    return float(ratio[m, t]), float(err[m, t]), float(bnd[m, t]), (m, t)


class Case(object):
    """the fp64 references, floor and bounds of a batch of rows under one bank; computed once, never modified"""

    def __init__(self, bank, wav, lens):
        self.bank, self.lens = bank, tuple(lens)
        self.wav = wav
        self.ref = [mel(wav[b], n, bank, torch.float64) for b, n in enumerate(lens)]
        self.floor = floor([mel(wav[b], n, bank, torch.float32) for b, n in enumerate(lens)], self.ref, bank)
        self.bound = [bound(bank, r, self.floor) for r in self.ref]

    def judge(self, out_log, mutation=None):
        """out_log (B, 80, >= T_b): the worst entry of the batch, (err / bound, err, bound, (b, m, t)).  With a mutation the
        device is held against the mutated fp64 reference under the un-mutated bounds."""
        worst = (-1.0, 0.0, 0.0, None)
        for b, n in enumerate(self.lens):
            T = n // HOP + 1
            ref = self.ref[b].mel if mutation is None else mel(self.wav[b], n, self.bank, torch.float64, mutation).mel
            r, e, bd, (m, t) = compare(out_log[b, :, :T], ref, self.bound[b])
            if r > worst[0]:
                worst = (r, e, bd, (b, m, t))
        return worst


# ------------------------------------------------------------------------------------------------ the cases both test files share
# the ragged batch: 513 is the minimum (T = 3, every frame reflects); T steps between 767 and 768; 3584, 3840 and 4096 give
# T = 15, 16, 17, one frame short of, exactly at and one over a workgroup; 20 * 1024 + 1 has interior frames, is odd, and sits
# in an odd row, as do 768, 1537 and 3840 with theirs
LENS = (513, 20 * 1024 + 1, 767, 768, 1025, 1537, 3584, 3840, 4096)

# (mutation, bank, signal) a mutation is asserted on
MUTATED = (tuple((m, bank, 'noise') for bank in (DEFAULT_BANK, FALLBACK_BANK) for m in MUTATIONS[:6])
           + tuple((m, DEFAULT_BANK, 'steptone') for m in ('edge', 'shift', 'symhann', 'mirror', 'tap_last'))
           + (('tap21', FALLBACK_BANK, 'tone'), ('tap41', FALLBACK_BANK, 'tone')))
MUTATED_IDS = ['%s-%s-%s' % (m, bank_name(bank), sig) for m, bank, sig in MUTATED]


def case(basis, sig, lens=LENS):
    return Case(basis, batch(sig, lens, k0_step=57), lens)


def mutation_case(basis, mutation, sig):
    """the batch a mutation is asserted on; a single-tap mutation gets a tone ON that tap's bin, because the edge taps of a
    triangle are faint on noise"""
    if sig != 'tone':
        return case(basis, sig)
    lens = (2048, 1537)
    wav = torch.zeros(2, 2048)
    for b, n in enumerate(lens):
        wav[b, :n] = signal('tone', n, seed=b, k0=tap_bin(basis, mutation)[1])
    return Case(basis, wav, lens)
