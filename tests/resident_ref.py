"""The test corpus of the resident-corpus tests (tests/test_resident_corpus.py, tests/test_resident_corpus_gpu.py).

Nine wavs of seeded noise: 513 samples is the smallest the front end takes, 767 / 768 / 769 sit around a hop boundary, and the
frame counts n // 256 + 1 spread from 3 to 17.  The texts have 1 to 6 Hangul syllables; two pairs have equal symbol counts
(rows 1, 2 and rows 3, 4, built from syllables of the same shape), and the longest text (row 5) is not on the longest wav
(row 8).  Speakers are all 0, emotions 0 to 3.  Rows 0..5 are the training list, rows 6..8 the validation list."""
import os

import numpy as np

SAMPLES = (513, 767, 768, 769, 1024, 2303, 2560, 4000, 4096)
TEXTS = ("가", "나다", "마바", "사아자", "차카타", "가나다라마바", "파하가나", "다라마바사", "강산")
EMOTIONS = tuple(i % 4 for i in range(9))
N_TRAIN = 6


def write_wav(path, n, seed, rate=16000):
    from scipy.io.wavfile import write
    g = np.random.RandomState(seed)
    write(path, rate, (np.clip(0.1 * g.randn(n), -1, 1) * 32767).astype(np.int16))


def write_corpus(root):
    """writes the wavs and both filelists under `root`; returns (training list, validation list, rows) with rows the nine
    (path, text, speaker, emotion) in file order"""
    root = str(root)
    rows = []
    for i, (n, text, emo) in enumerate(zip(SAMPLES, TEXTS, EMOTIONS)):
        path = os.path.join(root, 'u%d.wav' % i)
        write_wav(path, n, 100 + i)
        rows.append((path, text, 0, emo))
    lists = []
    for name, part in (('train.txt', rows[:N_TRAIN]), ('val.txt', rows[N_TRAIN:])):
        path = os.path.join(root, name)
        with open(path, 'w', encoding='utf-8') as f:
            f.write("".join("%s|%s|%d|%d\n" % r for r in part))
        lists.append(path)
    return lists[0], lists[1], rows


def hparams(train_list, val_list, extra=""):
    import hparams as HP
    return HP.create_hparams("anneal_function=constant,training_files=%s,validation_files=%s%s"
                             % (train_list, val_list, "," + extra if extra else ""))
