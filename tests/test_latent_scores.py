"""latent_scores (host arithmetic on what t2v_hip.latent_neighbours returns), tests/latent_ref.py itself, the command lines
of latent_report.py / extract_latents.py --scores / evaluate.py --style, and the style block of evaluation.summarize.
No GPU: the kernel's tests are tests/test_latent_gpu.py and tests/test_style_eval_gpu.py."""
import json
import os
import re

import numpy as np
import pytest

import latent_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _points(n=60, d=5, c=3, seed=3):
    rs = np.random.RandomState(seed)
    lab = np.arange(n) % c
    return rs.standard_normal((c, d))[lab] * 1.5 + rs.standard_normal((n, d)), lab


# ---------------------------------------------------------------------------------------------- the scores
def test_knn_predict_votes_and_breaks_ties_by_the_nearest():
    from latent_scores import knn_predict
    labels = np.array([0, 0, 1, 1, 2, 2, 3])
    idx = np.array([[0, 2, 1],          # 0, 1, 0 -> 0
                    [2, 0, 3],          # 1, 0, 1 -> 1
                    [4, 2, 0],          # 2, 1, 0: three-way tie -> the nearest's class, 2
                    [6, 4, 2],          # 3, 2, 1 -> 3
                    [0, 2, 4]])         # 0, 1, 2 -> 0
    assert knn_predict(idx, labels, 4).tolist() == [0, 1, 2, 3, 0]
    four = np.array([[2, 4, 5, 3],      # 1, 2, 2, 1: tie of 1 and 2 -> 1 (nearest)
                     [4, 2, 3, 5],      # 2, 1, 1, 2 -> 2
                     [0, 4, 5, 1]])     # 0, 2, 2, 0 -> 0
    assert knn_predict(four, labels, 4).tolist() == [1, 2, 0]
    assert knn_predict(np.array([[6]]), labels, 4).tolist() == [3]
    rs = np.random.RandomState(0)
    lab = rs.randint(0, 4, size=50)
    idx = np.array([rs.permutation(50)[:7] for _ in range(40)])
    assert knn_predict(idx, lab, 4).tolist() == R.knn_vote(idx, lab, 4).tolist()
    with pytest.raises(ValueError):
        knn_predict(np.array([0, 1]), labels, 4)
    with pytest.raises(ValueError):
        knn_predict(idx, lab, 3)


def test_silhouette_equals_the_direct_computation():
    from latent_scores import silhouette
    x, lab = _points()
    lab[7] = 3                                          # class 3: a singleton
    ref = R.neighbours(x, lab, k=3, n_classes=5)        # class 4 stays empty
    s = silhouette(ref.class_sum, ref.class_cnt, lab)
    want = R.silhouette_direct(x, lab)
    assert s.shape == (60,) and np.allclose(s, want, rtol=0, atol=1e-12)
    assert s[7] == 0.0 and -1 <= s.min() and s.max() <= 1 and 0.1 < s.mean() < 0.9
    # one class only: no other cluster to compare with
    one = R.neighbours(x, lab * 0, k=3, n_classes=1)
    assert np.isnan(silhouette(one.class_sum, one.class_cnt, lab * 0)).all()
    assert np.isnan(R.silhouette_direct(x, lab * 0)).all()
    # queries that are not among the references: own class = any label, nothing excluded
    q = x[:4] + 0.1
    cross = R.neighbours(x, lab, q, k=3, n_classes=5)
    s = silhouette(cross.class_sum, cross.class_cnt, np.array([0, 1, 2, 0]))
    d = np.sqrt(R.sq_distances(q, x))
    a, b = d[1, lab == 1].mean(), min(d[1, lab == c].mean() for c in (0, 2, 3))
    assert s[1] == pytest.approx((b - a) / max(a, b), abs=1e-12)
    with pytest.raises(ValueError):
        silhouette(ref.class_sum, ref.class_cnt[:, :4], lab)
    with pytest.raises(ValueError):
        silhouette(ref.class_sum, ref.class_cnt, lab + 3)


def test_confusion_active_units_and_kl():
    from latent_scores import active_units, confusion, kl_per_dim
    m = confusion([0, 0, 1, 2, 2, 2], [0, 1, 1, 2, 0, 2], 4)
    assert m.tolist() == [[1, 1, 0, 0], [0, 1, 0, 0], [1, 0, 2, 0], [0, 0, 0, 0]] and m.dtype == np.int64
    with pytest.raises(ValueError):
        confusion([0, 4], [0, 0], 4)
    with pytest.raises(ValueError):
        confusion([0, 1], [0], 4)
    # a hand-made corpus: 3 of 8 dimensions vary, the other five sit at the prior (mu = 0, logvar = 0)
    rs = np.random.RandomState(1)
    mus, logvars = np.zeros((200, 8)), np.zeros((200, 8))
    mus[:, [1, 4, 6]] = rs.standard_normal((200, 3)) * np.array([1.0, 0.5, 2.0])
    logvars[:, [1, 4, 6]] = -1.5
    assert active_units(mus) == 3 and active_units(mus, threshold=1.5) == 1 and active_units(mus * 0.01) == 0
    kl = kl_per_dim(mus, logvars)
    assert kl.shape == (8,) and (kl[[0, 2, 3, 5, 7]] == 0.0).all() and (kl[[1, 4, 6]] > 0.3).all()
    want = 0.5 * (mus[:, 6] ** 2 + np.exp(-1.5) + 1.5 - 1.0).mean()
    assert kl[6] == pytest.approx(want, rel=1e-12)
    with pytest.raises(ValueError):
        kl_per_dim(mus, logvars[:, :7])


def test_report_round_trips_through_json():
    from evaluation import EMOTIONS
    from latent_scores import report, summary_lines
    x, lab = _points(n=80, d=6, c=3)                    # emotion 3 ('hap') has no rows
    ref = R.neighbours(x, lab, k=5, n_classes=4)
    rs = np.random.RandomState(2)
    mus, logvars = rs.standard_normal((80, 6)), rs.standard_normal((80, 6)) * 0.1
    rep = report(ref.idx, ref.class_sum, ref.class_cnt, lab, mus, logvars)
    assert json.loads(json.dumps(rep)) == rep
    assert rep['n'] == 80 and rep['k'] == 5 and set(rep['by_emotion']) == set(EMOTIONS)
    pred = R.knn_vote(ref.idx, lab, 4)
    assert rep['knn_accuracy'] == pytest.approx((pred == lab).mean()) and 0.5 < rep['knn_accuracy'] <= 1
    assert rep['silhouette_mean'] == pytest.approx(R.silhouette_direct(x, lab).mean())
    assert np.array(rep['confusion']).sum() == 80 and np.trace(np.array(rep['confusion'])) == (pred == lab).sum()
    assert rep['by_emotion']['hap'] == {'n': 0, 'knn_accuracy': None, 'silhouette_mean': None}
    assert rep['by_emotion']['sad']['n'] == 27 and rep['by_emotion']['sad']['knn_accuracy'] == pytest.approx((pred == lab)[lab == 1].mean())
    assert rep['active_units'] == 6 and len(rep['kl_per_dim']) == 6 and rep['kl_total'] == pytest.approx(sum(rep['kl_per_dim']))
    lines = summary_lines(rep)
    assert len(lines) == 4 and 'kNN accuracy' in lines[0] and 'hap n/a' in lines[1] and 'active units 6 of 6' in lines[3]
    bare = report(ref.idx, ref.class_sum, ref.class_cnt, lab)
    assert 'active_units' not in bare and len(summary_lines(bare)) == 4
    with pytest.raises(ValueError):
        report(ref.idx[:10], ref.class_sum, ref.class_cnt, lab)


def test_reference_orders_by_distance_then_index():
    """tests/latent_ref.py on a case small enough to check by hand"""
    refs = np.array([[0.0, 0], [1, 0], [0, 1], [1, 1], [0, 0]])
    lab = np.array([0, 1, 0, 1, 1])
    r = R.neighbours(refs, lab, k=2, n_classes=2, target=[4, 0, -1, 0, 0])
    assert r.idx.tolist() == [[4, 1], [0, 3], [0, 3], [1, 2], [0, 1]]       # row 0: its copy 4 first, then the tie 1 < 2
    assert r.rank.tolist() == [1, 1, -1, 3, 0]                              # exclusion does not apply: row 0 itself precedes 4
    assert r.class_cnt.tolist() == [[1, 3], [2, 2], [1, 3], [2, 2], [2, 2]]
    assert r.class_sum[0].tolist() == [1.0, 1.0 + 2 ** 0.5]
    assert R.decided(r.d2, np.arange(5), 2).tolist() == [False] * 5
    assert R.neighbours(refs, lab, refs[:2], k=1, n_classes=2).idx.tolist() == [[0], [1]]


# ---------------------------------------------------------------------------------------------- command lines
def test_latent_report_parser():
    import latent_report as L
    a = L.parse_args(['--latents', 'in.npz', '--out', 'rep.json'])
    assert (a.latents, a.out, a.key, a.k) == ('in.npz', 'rep.json', 'mus', 5)
    a = L.parse_args(['--latents', 'in.npz', '--out', 'rep.json', '--key', 'zs', '--k', '9'])
    assert (a.key, a.k) == ('zs', 9)
    for bad in (['--k', '0'], ['--k', '33'], ['--k', 'x'], ['--key', 'prosody'], ['--key', 'logvars']):
        with pytest.raises(SystemExit):
            L.parse_args(['--latents', 'in.npz', '--out', 'rep.json'] + bad)
    with pytest.raises(SystemExit):
        L.parse_args(['--latents', 'in.npz'])


def test_latent_report_needs_the_arrays_of_extract_latents(tmp_path):
    import latent_report as L
    src = str(tmp_path / 'lat.npz')
    np.savez(src, zs=np.zeros((9, 4), np.float32), emotions=np.zeros(9, np.int64))
    with pytest.raises(SystemExit, match="mus, logvars"):
        L.main(['--latents', src, '--out', str(tmp_path / 'rep.json')])
    assert not os.path.exists(str(tmp_path / 'rep.json'))


class _FakeSynthesizer(object):
    def __init__(self, hp, **kw):
        pass

    def load_checkpoint(self, path):
        return self

    def latents(self, paths, batch_size):
        import torch
        g = torch.Generator().manual_seed(0)
        n = len(paths)
        return (torch.randn(n, 16, generator=g), torch.randn(n, 4, generator=g), torch.randn(n, 4, generator=g),
                torch.randn(n, 4, generator=g))


def test_extract_latents_scores_flag(tmp_path, monkeypatch):
    import extract_latents as X
    import latent_scores
    import synthesizer
    base = ['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.npz']
    assert X.parse_args(base).scores is None and X.parse_args(base).tsne is None
    assert X.parse_args(base + ['--scores']).scores == 'mus' and X.parse_args(base + ['--scores', 'zs']).scores == 'zs'
    for bad in ('prosody', 'logvars'):
        with pytest.raises(SystemExit):
            X.parse_args(base + ['--scores', bad])
    fl = tmp_path / 'f.txt'
    fl.write_text(''.join('w%d.wav|text|0|%d\n' % (i, i % 4) for i in range(6)), encoding='utf-8')
    monkeypatch.setattr(synthesizer, 'Synthesizer', _FakeSynthesizer)
    seen = []

    def fake_report(values, labels, mus=None, logvars=None, k=5):
        seen.append((values, labels, mus, logvars, k))
        return {'n': len(values), 'knn_accuracy': 0.5}
    monkeypatch.setattr(latent_scores, 'corpus_report', fake_report)
    plain, scored = str(tmp_path / 'plain.npz'), str(tmp_path / 'scored.npz')
    args = ['--load_path', 'ck', '--filelist_path', str(fl)]
    X.main(args + ['--out', plain])
    assert not seen
    with np.load(plain) as f:
        assert sorted(f.files) == ['emotions', 'logvars', 'mus', 'paths', 'prosody', 'zs']      # what it always was
        mus, zs, logvars = f['mus'], f['zs'], f['logvars']
    X.main(args + ['--out', scored, '--scores', 'zs'])
    with np.load(scored) as f:
        assert sorted(f.files) == ['emotions', 'logvars', 'mus', 'paths', 'prosody', 'scores', 'zs']
        assert json.loads(str(f['scores'])) == {'n': 6, 'knn_accuracy': 0.5}
        assert np.array_equal(f['mus'], mus)
    (values, labels, m, lv, k), = seen
    assert np.array_equal(values, zs) and labels.tolist() == [0, 1, 2, 3, 0, 1] and np.array_equal(m, mus) and np.array_equal(lv, logvars)
    assert k == 5


def test_evaluate_style_flags():
    import evaluate as E
    base = ['--load_path', 'ck', '--filelist_path', 'f.txt', '--out', 'o.json']
    a = E.parse_args(base)
    assert a.style is False and a.style_k == 5
    a = E.parse_args(base + ['--style', '--style_k', '3', '--prosody', '--alignment', '--condition', 'emotion'])
    assert a.style and a.style_k == 3 and a.prosody and a.alignment and a.condition == 'emotion'
    for bad in ('0', '33'):
        with pytest.raises(SystemExit):
            E.parse_args(base + ['--style', '--style_k', bad])


# ---------------------------------------------------------------------------------------------- C ABI, host-side checks
def test_latent_entries_are_declared_exported_and_bound():
    import t2v_hip
    with open(os.path.join(ROOT, 'include', 't2vae.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    protos = dict(re.findall(r'\b(t2v_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    lib = t2v_hip.load_library()
    for name in ('t2v_latent_scratch_bytes', 't2v_latent_neighbours'):
        assert name in protos and name in t2v_hip.EXPORTS and hasattr(lib, name), name
        assert protos[name].count(',') + 1 == len(getattr(lib, name).argtypes), name
    for define, value in (('MAX_POINTS', t2v_hip.LATENT_MAX_POINTS), ('MAX_CLASSES', t2v_hip.LATENT_MAX_CLASSES),
                          ('MAX_K', t2v_hip.LATENT_MAX_K), ('TILE', t2v_hip.LATENT_TILE)):
        assert int(re.search(r'#define\s+T2V_LATENT_%s\s+(\d+)' % define, src).group(1)) == value
    assert t2v_hip.LatentNeighbours._fields == ('idx', 'dist', 'class_sum', 'class_cnt', 'rank')


def test_latent_sizes_are_refused_before_any_launch():
    import torch
    import t2v_hip
    lib = t2v_hip.load_library()
    size = lib.t2v_latent_scratch_bytes
    a, b, c = size(130, 130, 4, 5, 0), size(1100, 1100, 4, 5, 0), size(16384, 16384, 8, 32, 0)
    assert 0 < a < b < c < 256 << 20
    assert size(1100, 1100, 4, 5, 128) > size(1100, 1100, 4, 5, 1152) > 0
    for bad in ((1, 40, 4, 5, 0), (16385, 40, 4, 5, 0), (40, 1, 4, 5, 0), (40, 16385, 4, 5, 0), (40, 40, 0, 5, 0), (40, 40, 9, 5, 0),
                (40, 40, 4, 0, 0), (40, 40, 4, 33, 0), (40, 40, 4, 5, 100), (40, 40, 4, 5, -128)):
        assert size(*bad) == 0, bad

    def call(N=600, D=32, Cn=4, M=600, k=5, rows=0):
        return lib.t2v_latent_neighbours(None, None, N, D, Cn, None, M, None, None, k, rows, None, None, None, None, None, None, None)
    for kw in (dict(N=1), dict(N=16385), dict(D=1), dict(D=65), dict(Cn=0), dict(Cn=9), dict(k=0), dict(k=33)):
        assert call(**kw) == -1, kw                     # T2V_ERR_DIMS
    assert call() == -2                                 # T2V_ERR_ARG: the null pointers
    with pytest.raises(t2v_hip.T2VHipError):
        t2v_hip.latent_neighbours(torch.zeros(100, 32), np.zeros(100, dtype=np.int64))
    with pytest.raises(ValueError, match="refs"):
        t2v_hip.latent_neighbours(np.zeros((100, 32), np.float32), np.zeros(100, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- evaluation.summarize
def _records():
    base = dict(dtw=1.0, n_frames=20, n_ref_frames=22, hit_max=False)
    style = [(0, 0, 0, 0.5, 0.4), (0, 1, 2, 1.5, -0.1), (1, 1, 0, 0.7, None), (2, None, None, None, None), (2, 2, 5, 2.0, 0.2),
             (1, 1, 1, 0.9, 0.3)]
    out = []
    for i, (emo, vote, rank, dist, sil) in enumerate(style):
        r = dict(base, emotion=emo, dtw=1.0 + i)
        r.update(style_emotion=vote, style_hit=None if vote is None else vote == emo, style_own_rank=rank, style_own_dist=dist,
                 style_silhouette=sil)
        out.append(r)
    return out


def test_summarize_adds_the_style_block_only_with_the_keys():
    from evaluation import STYLE_KEYS, StyleRecords, style_fields, summarize
    assert STYLE_KEYS == ('style_emotion', 'style_hit', 'style_own_rank', 'style_own_dist', 'style_silhouette')
    recs = _records()
    assert all(set(STYLE_KEYS) <= set(r) for r in recs)
    plain = [{k: v for k, v in r.items() if k not in STYLE_KEYS} for r in recs]
    s_plain, s = summarize(plain), summarize(recs)
    assert set(s_plain) == {'overall', 'by_emotion'} and set(s) == {'overall', 'by_emotion', 'style'}
    assert {k: s[k] for k in s_plain} == s_plain                                     # the rest is unchanged
    st = s['style']
    assert st['k'] is None and st['ref_accuracy'] is None and st['n_recordings'] is None
    o = st['overall']
    assert o['n_style'] == 5                                                         # the None row is counted out, not as a miss
    assert o['accuracy'] == pytest.approx(4 / 5) and o['rank0_share'] == pytest.approx(2 / 5) and o['rank_median'] == 1
    assert o['silhouette_mean'] == pytest.approx((0.4 - 0.1 + 0.2 + 0.3) / 4)
    by = st['by_emotion']
    assert by['neu']['n_style'] == 2 and by['neu']['accuracy'] == 0.5 and by['neu']['rank_median'] == 1.0
    assert by['sad'] == {'n_style': 2, 'accuracy': 1.0, 'rank0_share': 0.5, 'rank_median': 0.5, 'silhouette_mean': pytest.approx(0.3)}
    assert by['ang'] == {'n_style': 1, 'accuracy': 1.0, 'rank0_share': 0.0, 'rank_median': 5, 'silhouette_mean': pytest.approx(0.2)}
    assert by['hap'] == {'n_style': 0, 'accuracy': None, 'rank0_share': None, 'rank_median': None, 'silhouette_mean': None}
    assert st['confusion'] == [[1, 1, 0, 0], [0, 2, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    # what the recordings say about themselves travels with the records, or as an argument
    tagged = StyleRecords(recs)
    tagged.style_info = {'k': 3, 'n_recordings': 6, 'ref_accuracy': 0.75}
    assert tagged == recs
    st = summarize(tagged)['style']
    assert (st['k'], st['n_recordings'], st['ref_accuracy']) == (3, 6, 0.75) and st['overall'] == o
    assert summarize(recs, style_info={'k': 2, 'n_recordings': 4, 'ref_accuracy': 0.5})['style']['ref_accuracy'] == 0.5
    assert json.loads(json.dumps(summarize(tagged))) == summarize(tagged)
    # every row without style fields: the block is there and empty
    none = [dict(r, **style_fields(r['emotion'], None, None, None, None)) for r in plain]
    assert summarize(none)['style']['overall'] == {'n_style': 0, 'accuracy': None, 'rank0_share': None, 'rank_median': None,
                                                   'silhouette_mean': None}
    assert style_fields(1, 1, 0, 0.25, float('nan')) == {'style_emotion': 1, 'style_hit': True, 'style_own_rank': 0,
                                                         'style_own_dist': 0.25, 'style_silhouette': None}
    assert style_fields(1, np.int64(2), np.int32(4), np.float64(0.5), np.float64(-0.5))['style_hit'] is False
