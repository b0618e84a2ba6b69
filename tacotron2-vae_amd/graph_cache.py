"""Which batch shapes of the training step run as a captured HIP graph, and which eagerly: the policy behind TrainEngine.

The replay watchdog.  A captured step is a DAG of ~220 nodes and ROCm's graph executor decides how its branches share
the runtime's queues (four by default; the same graph replays in 11.3 ms on 4 queues, 13.5 ms on 6) — a replay that is SLOWER than
the same step issued eagerly means the executor serialised independent branches.  The second and third replay of every new graph are
timed with events, the step after them is issued EAGERLY once (a valid training step like any other — the warm-up executions before
the capture are no baseline: allocator growth and lazy initialisation make them several times slower) and timed the same way; a
graph that loses by more than WATCHDOG_MS (+ 5 %) is suspect: PROBE_CONFIRM more replays are timed (one slow pair of replays next to
one lucky eager step is noise, e.g. with a neighbour process on the GPU), and if the best of all still loses the graph is dropped and
the shape keeps running eagerly (two host syncs per captured shape at most).  Rank-local in a multi-rank job: replay-or-eager is
every rank's own choice already.

One record per shape key, one explicit phase per record:
    warming      no graph yet: the first `graph_after` sights run eagerly, every later one tries to capture
    probing      captured; the first PROBE_REPLAYS replays are timed (watchdog on)
    calibrating  timed replays in: the next sight is the eager comparison step (asked for again until one is reported)
    suspect      lost the comparison: PROBE_CONFIRM more replays are timed, then the verdict
    kept         decided: replays, never timed again
    dropped      decided: eager from now on, `verdict` = (replay ms, eager ms)

No torch, no t2v_hip: the owner hands in `new_event()` (an object with record / synchronize / elapsed_time) and `release(span)`
(gives a graph's error-ledger block back), so the whole policy runs on a CPU with fakes."""
import collections

EAGER, COMPARE, CAPTURE, REPLAY = 'eager', 'compare', 'capture', 'replay'     # what a sight of a shape becomes

Entry = collections.namedtuple('Entry', 'graph static out no_grad span')      # static: the tensors a batch is loaded into


class Record(object):
    __slots__ = ('sights', 'entry', 'timed', 'phase', 'verdict')

    def __init__(self):
        self.sights = 0             # sights without a graph
        self.entry = None
        self.timed = []             # (start, end) events of the timed replays; the first (executor set-up) is never counted
        self.phase = 'warming'
        self.verdict = None         # (replay ms, eager ms) of the comparison a suspect / dropped graph lost


class GraphCache(object):
    PROBE_REPLAYS = 3           # the first replay (executor set-up) is not counted
    PROBE_CONFIRM = 3           # replays timed behind the eager comparison step before a suspect graph is dropped
    WATCHDOG_MS = 0.5
    MAX_SEEN = 4096

    def __init__(self, new_event, release, graph_after, max_graphs, watchdog=True):
        self.new_event, self.release = new_event, release
        self.graph_after, self.max_graphs = graph_after, max_graphs
        self.watchdog = watchdog        # read when each decision is made: the owner may flip it at any time
        self.records = collections.OrderedDict()    # warming shapes in order of first sight, live graphs least recently replayed first
        self.fallbacks = 0
        self._deferred = []             # spans of dropped graphs: released at the top of the owner's next step

    def live(self):
        return {k: r.entry for k, r in self.records.items() if r.entry is not None}

    def verdicts(self):
        return {k: r.verdict for k, r in self.records.items() if r.phase == 'dropped'}

    def sight(self, key):
        """(EAGER | COMPARE | CAPTURE | REPLAY, the entry to load the batch into before a REPLAY).  CAPTURE: room has been made."""
        rec = self.records.get(key)
        if rec is None:
            rec = self.records[key] = Record()
        if rec.entry is not None:
            if rec.phase == 'calibrating' and self.watchdog:
                return COMPARE, None        # this one step runs eagerly and is timed; the owner reports it with compared()
            return REPLAY, rec.entry
        if rec.phase == 'dropped':
            return EAGER, None
        rec.sights += 1
        if rec.sights <= self.graph_after:
            self._trim()
            return EAGER, None
        # a ragged loader (shapes that recur now and then) must not pin max_graphs private pools for ever: the least recently
        # replayed graph (and its activation pool) goes when a new shape wants a slot — with its whole record, so a shape that
        # comes back is warmed up, captured and probed again
        live = [k for k, r in self.records.items() if r.entry is not None]
        for old in live[:max(0, len(live) - self.max_graphs + 1)]:
            self.release(self.records.pop(old).entry.span)
        return CAPTURE, None

    def store(self, key, graph, static, out, no_grad, span):
        rec = self.records[key]
        rec.entry, rec.phase, rec.timed = Entry(graph, static, out, no_grad, span), 'probing', []

    def replay(self, key, then, drag=None):
        """replay the graph of `key` and return then(entry) — what the owner launches right behind the replay.  The timed region
        ends BEFORE `then`: in the multi-rank graph engine that call runs the whole-arena all-reduce, whose duration depends on
        what the peer ranks are doing (warm-up, capture, their own calibration) — the watchdog compares what this rank's
        executor did with the graph, nothing else.  drag (tests): called between a timed replay and its end event"""
        rec = self.records[key]
        self.records.move_to_end(key)       # most recently used last
        entry = rec.entry
        if not (self.watchdog and rec.phase in ('probing', 'suspect')):
            entry.graph.replay()
            return then(entry)
        t0 = self.new_event()
        t0.record()
        entry.graph.replay()
        if drag is not None:
            drag()
        t1 = self.new_event()
        t1.record()
        out = then(entry)
        rec.timed.append((t0, t1))
        if rec.phase == 'probing':
            if len(rec.timed) == self.PROBE_REPLAYS:
                rec.phase = 'calibrating'
        elif len(rec.timed) == self.PROBE_REPLAYS + self.PROBE_CONFIRM:
            t1.synchronize()
            self._judge(key, rec, rec.verdict[1])
        return out

    def compared(self, key, e0, e1):
        """the eager comparison step of `key` ran between the events e0 and e1"""
        rec = self.records.get(key)
        if rec is not None and rec.phase == 'calibrating':
            e1.synchronize()
            self._judge(key, rec, e0.elapsed_time(e1))

    def _judge(self, key, rec, eager_ms):
        replay_ms = min(a.elapsed_time(b) for a, b in rec.timed[1:])
        lost = replay_ms > eager_ms * 1.05 + self.WATCHDOG_MS
        if lost and rec.phase == 'calibrating':
            rec.phase, rec.verdict = 'suspect', (replay_ms, eager_ms)
            return
        n, rec.timed = len(rec.timed) - 1, []       # (events released)
        if not lost:
            rec.phase, rec.verdict = 'kept', None
            return
        # NOT released here: this is the graph that was replayed in this very step — its block holds the step's error words until
        # the caller's check has run (flush_released() at the top of the next step)
        self._deferred.append(rec.entry.span)
        rec.entry, rec.phase, rec.verdict = None, 'dropped', (replay_ms, eager_ms)
        self.records.move_to_end(key)       # (verdicts in the order they fell)
        self.fallbacks += 1
        print("TrainEngine: the captured graph of this batch shape replays in %.2f ms (best of %d), the same step issued eagerly takes "
              "%.2f ms — the graph executor serialised independent branches; the shape keeps running eagerly" % (
                  replay_ms, n, eager_ms), flush=True)

    def flush_released(self):
        while self._deferred:
            self.release(self._deferred.pop())

    def clear(self):
        """every block goes back to the free list, every record and verdict is forgotten"""
        for rec in self.records.values():
            if rec.entry is not None:
                self.release(rec.entry.span)
        self.records.clear()
        self.flush_released()

    def _trim(self):
        """the shape history is bounded (one record per distinct batch shape otherwise, for the whole run): the oldest half of the
        records without a graph goes, and the oldest half of the verdicts on its own"""
        if len(self.records) <= self.MAX_SEEN:
            return
        cold = [k for k, r in self.records.items() if r.phase == 'warming']
        gone = [k for k, r in self.records.items() if r.phase == 'dropped']
        for keys in (cold, gone if len(gone) > self.MAX_SEEN else ()):
            for k in keys[:len(keys) // 2]:
                del self.records[k]
