"""graph_cache.GraphCache on the CPU: which sight of a batch shape runs eagerly, captures, replays, is timed or is the watchdog's
eager comparison step.  A fake clock stamps fake events, fake graphs advance the clock by the duration the case gives them and
count their replays, `release` appends to a list.  Each case drives the cache the way TrainEngine._step / _graph_step do and
asserts the sequence of actions with its timed / untimed pattern."""
import inspect
import math

import pytest

import graph_cache as GC


class Bench(object):
    """the owner's side of the interface, with fakes"""

    def __init__(self, **kw):
        self.now = 0.0
        self.log = []               # 'then' / 'sync' in the order they happened
        self.released = []
        self.events = 0
        self.spans = 0
        self.cache = GC.GraphCache(self.new_event, self.released.append, kw.pop('graph_after', 2), kw.pop('max_graphs', 8), **kw)

    def new_event(self):
        bench = self
        bench.events += 1

        class Event(object):
            def record(self):
                self.t = bench.now

            def synchronize(self):
                bench.log.append('sync')

            def elapsed_time(self, other):
                return other.t - self.t
        return Event()

    def graph(self):
        bench = self

        class Graph(object):
            ms, replays = 0.0, 0

            def replay(self):
                self.replays += 1
                bench.now += self.ms
        return Graph()

    def sight(self, key, replay_ms=5.0, eager_ms=5.0, capture_ok=True, report=True):
        """one training step on a batch of shape `key`; returns what it became"""
        self.cache.flush_released()
        what, entry = self.cache.sight(key)
        if what == GC.COMPARE:
            e0, e1 = self.new_event(), self.new_event()
            e0.record()
            self.now += eager_ms
            e1.record()
            if report:
                self.cache.compared(key, e0, e1)
            return 'compare'
        if what == GC.CAPTURE:
            if not capture_ok:
                return 'capture failed'
            self.spans += 1
            self.cache.store(key, self.graph(), ['static of %r' % (key,)], ('out',), None, 'span%d' % self.spans)
        elif what == GC.REPLAY:
            assert entry is self.cache.live()[key] and entry.static == ['static of %r' % (key,)]
        else:
            assert what == GC.EAGER
            return 'eager'
        graph, span = self.cache.records[key].entry.graph, self.cache.records[key].entry.span
        graph.ms = replay_ms
        n, events = graph.replays, self.events
        assert self.cache.replay(key, self.then) == ('then', span)      # what the owner launched behind the replay comes back
        assert graph.replays == n + 1
        assert self.events - events in (0, 2)
        return ('capture+' if what == GC.CAPTURE else '') + ('timed' if self.events > events else 'replay')

    def then(self, entry):
        self.log.append('then')
        return 'then', entry.span

    def run(self, key, n, **kw):
        return [self.sight(key, **kw) for _ in range(n)]


def test_entry_is_one_named_record_and_the_module_needs_no_torch():
    assert GC.Entry._fields == ('graph', 'static', 'out', 'no_grad', 'span')
    src = inspect.getsource(GC)
    assert 'import torch' not in src and 'import t2v_hip' not in src


def test_healthy_shape_is_probed_compared_once_and_kept():
    b = Bench()
    assert b.run('A', 9) == ['eager', 'eager', 'capture+timed', 'timed', 'timed', 'compare', 'replay', 'replay', 'replay']
    rec = b.cache.records['A']
    assert rec.phase == 'kept' and rec.verdict is None and rec.timed == []
    assert b.log.count('sync') == 1 and 'sync' not in b.log[b.log.index('sync') + 1:]      # the decision's, none behind it
    assert b.cache.fallbacks == 0 and b.released == [] and list(b.cache.live()) == ['A'] and not b.cache.verdicts()


def test_slow_graph_is_suspect_then_dropped_and_its_span_waits_for_the_next_step(capsys):
    b = Bench()
    ms = [0.0, 0.0, 10.0, 10.0, 10.0, 0.0, 11.0, 9.0, 12.0]     # replay_ms: 2 warm-ups, replays 1-3, the comparison step, replays 4-6
    got = [b.sight('A', replay_ms=m, eager_ms=5.0) for m in ms]
    assert got == ['eager', 'eager', 'capture+timed', 'timed', 'timed', 'compare', 'timed', 'timed', 'timed']
    assert b.log[-2:] == ['then', 'sync']               # the confirming synchronise comes behind what the owner launched
    assert b.log.count('sync') == 2
    rec = b.cache.records['A']
    assert rec.phase == 'dropped' and rec.entry is None and b.cache.fallbacks == 1
    assert b.cache.verdicts() == {'A': (9.0, 5.0)}      # best of replays 2-6 (the first is never counted), eager
    assert not b.cache.live()
    assert b.released == []                             # its block still holds this step's error words
    assert capsys.readouterr().out == (
        "TrainEngine: the captured graph of this batch shape replays in 9.00 ms (best of 5), the same step issued eagerly takes "
        "5.00 ms — the graph executor serialised independent branches; the shape keeps running eagerly\n")
    b.cache.flush_released()
    assert b.released == ['span1']
    assert b.run('A', 3) == ['eager'] * 3 and b.released == ['span1'] and b.cache.records['A'].sights == 3


def test_suspect_graph_that_wins_the_confirmation_is_kept():
    b = Bench()
    assert b.run('A', 5, replay_ms=10.0) == ['eager', 'eager', 'capture+timed', 'timed', 'timed']
    assert b.sight('A', eager_ms=5.0) == 'compare'
    assert b.cache.records['A'].phase == 'suspect' and b.cache.records['A'].verdict == (10.0, 5.0)
    assert not b.cache.verdicts()                       # (a suspect's lost comparison is no verdict yet)
    assert b.run('A', 5, replay_ms=4.0) == ['timed', 'timed', 'timed', 'replay', 'replay']
    rec = b.cache.records['A']
    assert rec.phase == 'kept' and rec.verdict is None and rec.timed == []
    assert b.cache.fallbacks == 0 and b.released == [] and list(b.cache.live()) == ['A'] and not b.cache.verdicts()
    b.cache.flush_released()
    assert b.released == []


def test_first_replay_is_never_counted():
    b = Bench()
    b.run('A', 2)
    assert [b.sight('A', replay_ms=m) for m in (100.0, 5.0, 5.0)] == ['capture+timed', 'timed', 'timed']
    assert b.sight('A', eager_ms=5.0) == 'compare'
    assert b.cache.records['A'].phase == 'kept'         # never suspect
    assert b.run('A', 3) == ['replay'] * 3


@pytest.mark.parametrize('above', [False, True])
def test_threshold_is_five_percent_plus_watchdog_ms(above):
    eager = 7.3
    limit = eager * 1.05 + GC.GraphCache.WATCHDOG_MS
    replay = math.nextafter(limit, math.inf) if above else limit
    b = Bench()
    b.run('A', 2)
    for _ in range(3):
        b.now = 0.0                                     # (stamps 0 and `replay`: the difference is exact)
        assert b.sight('A', replay_ms=replay).endswith('timed')
    b.now = 0.0
    assert b.sight('A', eager_ms=eager) == 'compare'
    assert b.cache.records['A'].phase == ('suspect' if above else 'kept')


def test_watchdog_off_times_nothing_and_never_compares():
    b = Bench()
    b.cache.watchdog = False                            # flipped after construction, as the engine's owner does
    assert b.run('A', 12, replay_ms=50.0) == ['eager', 'eager', 'capture+replay'] + ['replay'] * 9
    assert b.events == 0 and 'sync' not in b.log and b.cache.records['A'].phase == 'probing'
    b.cache.watchdog = True                             # ... and it is read at every decision: probing starts now
    assert b.run('A', 4) == ['timed', 'timed', 'timed', 'compare']


def test_least_recently_replayed_graph_is_evicted_with_its_whole_record():
    b = Bench(max_graphs=2)
    b.cache.watchdog = False
    b.run('A', 3)
    b.run('B', 3)
    assert b.sight('A') == 'replay' and list(b.cache.live()) == ['B', 'A']
    assert b.run('C', 2) == ['eager', 'eager'] and b.released == []
    assert b.sight('C') == 'capture+replay'
    assert b.released == ['span2'] and 'B' not in b.cache.records and list(b.cache.live()) == ['A', 'C']
    assert b.run('B', 2) == ['eager', 'eager'] and b.released == ['span2']
    assert b.sight('B') == 'capture+replay'             # ... and A, the least recently replayed by now, made room for it
    assert b.released == ['span2', 'span1'] and list(b.cache.live()) == ['C', 'B']


def test_failed_capture_runs_eagerly_and_is_tried_again_at_the_next_sight():
    b = Bench(max_graphs=1)
    b.run('A', 3)
    b.run('B', 2)
    assert b.sight('B', capture_ok=False) == 'capture failed'
    assert b.released == ['span1']                      # room is made in front of every attempt
    assert b.cache.records['B'].phase == 'warming' and not b.cache.live()
    assert b.sight('B', capture_ok=False) == 'capture failed'
    assert b.run('B', 2) == ['capture+timed', 'timed'] and b.released == ['span1']


def test_clear_releases_every_span_and_forgets_verdicts_and_a_pending_comparison():
    b = Bench()
    b.run('A', 5)
    b.run('B', 3)
    b.run('D', 5, replay_ms=10.0)
    b.run('D', 4, replay_ms=10.0, eager_ms=5.0)         # dropped in this step: its span waits
    assert b.cache.verdicts() and b.released == []
    assert b.cache.sight('A') == (GC.COMPARE, None)     # a comparison step that is on its way
    syncs = b.log.count('sync')
    b.cache.clear()
    assert sorted(b.released) == ['span1', 'span2', 'span3']
    assert not b.cache.records and not b.cache.live() and not b.cache.verdicts()
    e0, e1 = b.new_event(), b.new_event()
    e0.record(), e1.record()
    b.cache.compared('A', e0, e1)                       # the report of that step finds nothing to decide
    assert not b.cache.records and b.log.count('sync') == syncs
    b.cache.clear()
    assert len(b.released) == 3                         # nothing is released twice
    assert b.run('D', 3) == ['eager', 'eager', 'capture+timed']     # a dropped shape gets another chance


def test_comparison_that_was_not_reported_is_asked_for_again():
    b = Bench()
    b.run('A', 5)
    assert b.sight('A', report=False) == 'compare'
    assert b.cache.records['A'].phase == 'calibrating'
    assert b.sight('A', report=False) == 'compare'
    assert b.run('A', 2) == ['compare', 'replay'] and b.cache.records['A'].phase == 'kept'


def test_history_is_trimmed_to_its_newer_half_and_live_graphs_stay():
    b = Bench()
    b.cache.MAX_SEEN = 8
    b.run('live', 3)
    for k in range(1, 8):
        b.run(k, 2 if k == 5 else 1)
    assert len(b.cache.records) == 8                    # not above the bound yet
    b.sight(8)
    assert list(b.cache.records) == ['live', 5, 6, 7, 8]        # the oldest half of the eight graph-less records went
    assert b.sight('live') == 'timed'
    assert b.sight(5) == 'capture+timed'                # its two warm-up sights are remembered
    assert b.run(1, 3) == ['eager', 'eager', 'capture+timed']   # a forgotten shape starts again


def test_verdicts_are_bounded_on_their_own():
    b = Bench()
    b.cache.MAX_SEEN = 2
    for k in ('D1', 'D2', 'D3'):
        b.run(k, 5, replay_ms=10.0)
        b.run(k, 4, replay_ms=10.0, eager_ms=5.0)
    assert list(b.cache.verdicts()) == ['D1', 'D2', 'D3']
    assert b.sight('new') == 'eager'
    assert list(b.cache.verdicts()) == ['D2', 'D3'] and b.cache.records['new'].sights == 1
    assert b.sight('D1') == 'eager' and b.cache.records['D1'].phase == 'warming'
