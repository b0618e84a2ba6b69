"""Reading RIFF wavs at any rate for the device resampler (t2v_hip.resample), and the two switches the command lines that
read wavs share: --resample and --trim_db (synthesizer.py, evaluate.py, extract_latents.py).  Host side only: numpy and scipy."""
import numpy as np

DEFAULT_TRIM_DB = 40.0
DEFAULT_PAD_FRAMES = 2


def add_wav_arguments(parser):
    """--resample and --trim_db DB on a command line that reads wavs; `wav_options(args)` gives Synthesizer's keywords"""
    parser.add_argument('--resample', action='store_true',
                        help="take wavs at any sampling rate: they are resampled to hparams.sampling_rate on the device "
                             "(without it a wav at another rate is an error)")
    parser.add_argument('--trim_db', type=float, default=None, metavar='DB',
                        help="trim leading and trailing silence: frames more than DB dB below the wav's loudest frame "
                             "(e.g. %g); off by default" % DEFAULT_TRIM_DB)
    return parser


def wav_options(args):
    """Synthesizer(hparams, **wav_options(args))"""
    if args.trim_db is not None and not 0.0 < args.trim_db < float('inf'):
        raise SystemExit("--trim_db must be a positive number of dB")
    return dict(resample=bool(args.resample), trim_db=args.trim_db)


def wav_header(path):
    """(sampling rate, samples per channel, channels) of a wav; the data is memory-mapped, not read"""
    from scipy.io.wavfile import read
    rate, data = read(path, mmap=True)
    return int(rate), int(data.shape[0]), (1 if data.ndim == 1 else int(data.shape[1]))


def read_wav(path):
    """(sampling rate, samples) of a mono wav for the device: int16 PCM as it lies in the file (the resampler scales it by
    1 / 32768 as it loads), int32 and float32 / float64 as float32 in [-1, 1) (int32 scaled by 2^-31 on the host).
    ValueError for more than one channel, an empty file or another sample format (8-bit, 24-bit)."""
    from scipy.io.wavfile import read
    rate, data = read(path)
    if data.ndim != 1:
        raise ValueError("%s: %d channels; only mono wavs are read" % (path, data.shape[1]))
    if data.shape[0] < 1:
        raise ValueError("%s: no samples" % (path,))
    if data.dtype == np.int16:
        return int(rate), np.ascontiguousarray(data)
    if data.dtype == np.int32:
        return int(rate), (data.astype(np.float64) * (1.0 / 2147483648.0)).astype(np.float32)
    if data.dtype in (np.float32, np.float64):
        return int(rate), data.astype(np.float32)
    raise ValueError("%s: sample format %s; int16, int32 and float wavs are read" % (path, data.dtype))
