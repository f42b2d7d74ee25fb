"""Coordinator job-state tables and the c1/c2/c4/cq/cvm views.

Table layouts are kept identical to the reference so the shell output and the
standby snapshot look the same (mp4_machinelearning.py:115-160):

  worker_set        {(model, qnum): [(worker, start, end, 'w'|'f', t_start, t_end), ...]}   (cq)
  working_vm_set    {worker: [(model, qnum, start, end), ...]}                              (cvm)
  inference_result_list {"<model> <qnum>": [str([(img, category, prob), ...]), ...]}      (c4 -> result.txt)
  query_processing_time_meta {model: [mean, q1, q2, q3, std]}                               (c2)

Deliberate fixes:
  A2  c1/c2 numbers are measured for *every* model (none synthesised from the other)
  A3  finished-image counts are end - start + 1
  A4  results are kept as arrays (class id int32, prob fp32) and rendered to
      the reference's string format lazily, so no 4 KB truncation exists
  A11 query numbers are coordinator-assigned
  A13 single writer: every mutation goes through this object under one lock,
      and result ingestion is idempotent by chunk key (model, qnum, start, end)

Standby replication (reference send_metadata pushes str() dumps
of every table every second, mp4_machinelearning.py:971-1011): every mutation
bumps ``seq`` and appends ``(seq, op, args)`` to a bounded log.  The
coordinator pushes only the entries after the standby's acknowledged sequence
number (``deltas_since``); the standby applies them in order
(``apply_deltas``) and asks for a full snapshot only when it sees a gap or the
log has been truncated past its position.  Queries whose chunks are all
finished leave the open-query index, so ``pending()`` and the scheduler's
per-submit scans are O(open work), not O(history).
"""
from __future__ import annotations

import json
import time
from collections import defaultdict, deque
from dataclasses import dataclass

import numpy as np

from ..utils import racecheck

WINDOW_S = 30.0  # reference SLIDING_WINDOW_SECONDS * SLIDING_WINDOW_FACTOR (10 * 3)

DEFAULT_BATCHSIZE = {"resnet18": 400, "alexnet": 500, "resnet50": 1024, "resnet34": 400,
                     # the rest of the ResNet family at the reference's query size
                     "resnet101": 400, "resnet152": 400, "resnext50_32x4d": 400, "resnext101_32x8d": 400,
                     "wide_resnet50_2": 400, "wide_resnet101_2": 400}


def class_names(n: int = 1000, path: str | None = None) -> list[str]:
    """ImageNet category names if a classes file is available, else synthetic.

    The reference downloads imagenet_classes.txt (alexnet_resnet.py:27-42);
    there is no network here, so a local file is optional."""
    import os

    cands = [path] if path else []
    cands.append(os.environ.get("IDUNNO_CLASSES", ""))
    for p in cands:
        if p and os.path.exists(p):
            with open(p) as f:
                names = [ln.strip() for ln in f if ln.strip()]
            if len(names) >= n:
                return names[:n]
    return [f"class_{i}" for i in range(n)]


@dataclass
class ChunkResult:
    start: int
    end: int
    cls: np.ndarray      # int32 [n]
    prob: np.ndarray     # float32 [n]
    worker: str

    def render(self, names: list[str]) -> str:
        tup = [(f"test_{self.start + i}.JPEG", names[int(c)] if 0 <= int(c) < len(names) else str(int(c)),
                float(p)) for i, (c, p) in enumerate(zip(self.cls.tolist(), self.prob.tolist()))]
        return str(tup)


def _add_interval(ivs: list, s: int, e: int) -> int:
    """Merge [s, e] into the sorted, disjoint interval list ``ivs`` (in place);
    returns how many of its integers were not already covered."""
    new = e - s + 1
    out, i = [], 0
    while i < len(ivs) and ivs[i][1] < s - 1:
        out.append(ivs[i])
        i += 1
    lo, hi = s, e
    while i < len(ivs) and ivs[i][0] <= e + 1:
        a, b = ivs[i]
        new -= max(0, min(b, e) - max(a, s) + 1)
        lo, hi = min(lo, a), max(hi, b)
        i += 1
    out.append([lo, hi])
    out.extend(ivs[i:])
    ivs[:] = out
    return new


class JobState:
    # tables the race detector watches (all mutated only under self.lock)
    _TABLES = ("worker_set", "working_vm_set", "results", "finished_images", "finished_queries",
               "next_qnum", "jobs", "query_latency", "query_submit_time")

    def __init__(self, batchsize: dict | None = None, clock=time.time, window_s: float = WINDOW_S,
                 names: list[str] | None = None):
        self.lock = racecheck.make_lock("jobstate", reentrant=True)
        self.clock = clock
        self.window_s = window_s
        self.batchsize = dict(DEFAULT_BATCHSIZE, **(batchsize or {}))
        self.names = names
        self.worker_set: dict = defaultdict(list)
        self.working_vm_set: dict = defaultdict(list)
        self.results: dict = defaultdict(list)          # "model q" -> [ChunkResult]
        self._done_keys: set = set()
        self._done_imgs: dict = defaultdict(list)       # (model, qnum) -> merged finished [s, e] ranges
        self.finished_images: dict = defaultdict(int)
        self.finished_queries: dict = defaultdict(int)
        self._rate_win: dict = defaultdict(deque)       # model -> (t_finish, n_images)
        self._ptime_win: dict = defaultdict(deque)      # model -> (t_finish, normalised query time)
        self.query_processing_time_meta: dict = {}
        self._c2_dirty: set = set()                     # models whose c2 stats are stale
        self.next_qnum: dict = defaultdict(int)
        self.seq = 0                                    # mutation counter (standby replication)
        self.query_submit_time: dict = {}
        self.query_latency: dict = defaultdict(list)    # model -> [end-to-end seconds]
        self.jobs: dict = {}                            # job id -> {model, start, end, next}
        # compaction indexes: (model, qnum) -> number of 'w' entries (only open queries),
        # and the (model, first start, last end) span of every submitted query
        self._open: dict = {}
        self._spans: set = set()
        # replication log: (seq, op, args) for every mutation since log_base
        self._log: list = []
        self._log_base = 0                              # seq of the entry before _log[0]
        self.log_cap = 100_000
        self.mirror_seq = 0                             # standby: last coordinator seq applied
        racecheck.instrument(self, self._TABLES)

    # -- replication log ------------------------------------------------------------
    def _bump(self, op: str, *args) -> None:
        """One mutation: seq + 1 and its log entry (caller holds the lock)."""
        self.seq += 1
        self._log.append((self.seq, op, args))
        if len(self._log) > self.log_cap:              # truncate: a standby that far behind re-syncs
            drop = len(self._log) - self.log_cap // 2
            self._log_base = self._log[drop - 1][0]
            del self._log[:drop]

    def deltas_since(self, seq: int) -> list | None:
        """Log entries after ``seq`` (oldest first), or None when the log no
        longer reaches back that far (the caller sends a full snapshot)."""
        with self.lock:
            if seq >= self.seq:
                return []
            if seq < self._log_base or not self._log:
                return None
            i = seq - self._log_base                    # entries are consecutive seqs
            if i < 0 or i >= len(self._log) or self._log[i][0] != seq + 1:
                return None
            return [list(e) for e in self._log[i:]]

    def _open_add(self, key, n: int) -> None:
        v = self._open.get(key, 0) + n
        if v > 0:
            self._open[key] = v
        else:
            self._open.pop(key, None)

    def _mark_finished(self, key, start: int, end: int, now: float):
        """'w' -> 'f' for the chunk [start, end] of query ``key``; returns the
        (worker, t_start) of the entry it closed, or None."""
        entries = self.worker_set.get(key, [])
        for i, ent in enumerate(entries):
            if ent[1] == start and ent[2] == end and ent[3] == "w":
                w, s, e, _, t_start, _ = ent
                entries[i] = (w, s, e, "f", t_start, now)
                try:
                    self.working_vm_set[w].remove((key[0], key[1], s, e))
                except ValueError:
                    pass
                if not self.working_vm_set[w]:
                    self.working_vm_set.pop(w, None)
                self._open_add(key, -1)
                return w, t_start
        return None

    def apply_deltas(self, entries: list) -> bool:
        """Standby: apply coordinator log entries in order (entries at or below
        ``mirror_seq`` are skipped, so re-sends are harmless).  Returns False on
        a gap (the coordinator then sends a full snapshot)."""
        with self.lock:
            for seq, op, args in entries:
                if seq <= self.mirror_seq:
                    continue
                if seq != self.mirror_seq + 1:
                    return False
                self._apply_one(op, args)
                self.mirror_seq = seq
            return True

    def _apply_one(self, op: str, args) -> None:
        if op == "qnum":
            m, v = args
            self.next_qnum[m] = max(self.next_qnum.get(m, 0), int(v))
        elif op == "job":
            jid, job, (m, v) = args
            cur = self.jobs.get(jid)
            if cur is None or job["next"] > cur["next"]:
                self.jobs[jid] = dict(job)
            self.next_qnum[m] = max(self.next_qnum.get(m, 0), int(v))
        elif op == "advance":
            jid, nxt = args
            if jid in self.jobs:
                self.jobs[jid]["next"] = max(self.jobs[jid]["next"], int(nxt))
        elif op == "assign":
            model, qnum, chunks, now = args
            self._assign_locked(model, qnum, chunks, now, emit=False)
        elif op == "result":
            model, qnum, start, end, now = args
            self._mark_finished((model, qnum), int(start), int(end), now)
        elif op == "results":                           # one collective round (record_results bulk)
            model, qnum, chunks, now = args
            for start, end in chunks:
                self._mark_finished((model, qnum), int(start), int(end), now)
        elif op == "reassign":
            failed, new_worker, chunk, now = args
            self._reassign_locked(failed, new_worker, tuple(chunk), now, emit=False)
        elif op == "reopen":
            self._reopen_locked(emit=False)
        elif op == "replan":
            model, qnum, old, new, now = args
            self._replan_locked(model, qnum, old, new, now, emit=False)
        # "noop" (a duplicate result) changes nothing

    # -- coordinator-side jobs (C28 variant), replicated to the standby ----------
    def add_job(self, model: str, start: int, end: int, bs: int | None = None) -> int:
        """Register a coordinator-side job and reserve the query numbers of all
        its batch-size queries up front (query k of the job is ``qbase + k``).
        A promoted standby that resumes the job from a lagging snapshot then
        re-issues a query the dead coordinator had already dispatched under the
        SAME number, and ``record_result``'s per-query image dedupe keeps the
        late results of the original dispatch from being counted twice."""
        bs = int(bs or self.batchsize.get(model, 1))
        with self.lock:
            jid = len(self.jobs) + 1
            nq = (int(end) - int(start)) // bs + 1
            qbase = self.next_qnum[model] + 1
            self.next_qnum[model] += nq
            self.jobs[jid] = {"model": model, "start": int(start), "end": int(end), "next": int(start),
                              "bs": bs, "qbase": qbase}
            self._bump("job", jid, dict(self.jobs[jid]), (model, self.next_qnum[model]))
            return jid

    def images_held(self, model: str, qnum, s: int, e: int) -> bool:
        """True if results for every image of [s, e] under (model, qnum) are held."""
        with self.lock:
            return any(a <= s and e <= b for a, b in self._done_imgs.get((model, qnum), []))

    def job_query_number(self, jid: int, s: int) -> int:
        with self.lock:
            j = self.jobs[jid]
            return j["qbase"] + (int(s) - j["start"]) // j["bs"]

    def advance_job(self, jid: int, nxt: int) -> None:
        with self.lock:
            self.jobs[jid]["next"] = int(nxt)
            self._bump("advance", jid, int(nxt))

    def unfinished_jobs(self) -> list[int]:
        with self.lock:
            return [j for j, v in self.jobs.items() if v["next"] <= v["end"]]

    def range_submitted(self, model: str, s: int, e: int) -> bool:
        """True if some query of ``model`` already covers exactly [s, e] chunks
        (used when a promoted standby resumes a job from a lagging snapshot)."""
        with self.lock:
            return (model, int(s), int(e)) in self._spans

    # -- ids --------------------------------------------------------------------
    def new_query_number(self, model: str) -> int:
        """Coordinator-assigned query number (fix A11; the reference counted on the client)."""
        with self.lock:
            self.next_qnum[model] += 1
            self._bump("qnum", model, self.next_qnum[model])
            return self.next_qnum[model]

    # -- mutations --------------------------------------------------------------
    def assign(self, model: str, qnum, chunks, now: float | None = None) -> None:
        """Record a dispatched query: chunks = [(worker, start, end), ...]."""
        now = self.clock() if now is None else now
        with self.lock:
            self._assign_locked(model, qnum, chunks, now, emit=True)

    def _assign_locked(self, model, qnum, chunks, now, emit: bool) -> None:
        key = (model, qnum)
        self.query_submit_time.setdefault(key, now)
        ents = self.worker_set[key]
        done, vms = self._done_keys, self.working_vm_set
        log, n_open = [], 0
        lo = hi = None
        for w, s, e in chunks:
            s, e = int(s), int(e)
            log.append([w, s, e])
            lo = s if lo is None or s < lo else lo
            hi = e if hi is None or e > hi else hi
            if (model, qnum, s, e) in done:                # mirror: result already held
                ents.append((w, s, e, "f", now, now))
                continue
            ents.append((w, s, e, "w", now, now))
            vms[w].append((model, qnum, s, e))
            n_open += 1
        if n_open:
            self._open_add(key, n_open)
        if ents:
            if len(ents) > len(log):                       # earlier entries of this query too
                lo, hi = min(x[1] for x in ents), max(x[2] for x in ents)
            self._spans.add((model, lo, hi))
        if emit:
            self._bump("assign", model, qnum, log, now)

    def record_result(self, model: str, qnum, worker: str, start: int, end: int, cls, prob,
                      now: float | None = None) -> bool:
        """Ingest one finished chunk.  Idempotent: returns False for duplicates
        (e.g. a re-dispatched chunk whose original worker also answered)."""
        now = self.clock() if now is None else now
        start, end = int(start), int(end)
        with self.lock:
            ck = (model, qnum, start, end)
            key = (model, qnum)
            entries = self.worker_set.get(key, [])
            was_done = bool(entries) and key not in self._open
            # a duplicate still closes a matching 'w' entry (a re-dispatch with the
            # same chunk boundaries as the answered original) before it is dropped
            hit = self._mark_finished(key, start, end, now)
            t_start = hit[1] if hit is not None else now
            dup = ck in self._done_keys
            self._done_keys.add(ck)
            if entries and not was_done and key not in self._open:
                self.finished_queries[model] += 1
                t0 = self.query_submit_time.get(key)
                if t0 is not None:
                    self.query_latency[model].append(now - t0)
            # images of this query already answered under another chunk split
            # (re-dispatch after a failure / a resumed job) are not counted again
            n = 0 if dup else _add_interval(self._done_imgs[key], start, end)   # fix A3: end-start+1 when new
            if n == 0:
                self._bump("result" if hit is not None else "noop", model, qnum, start, end, now)
                return False
            self.finished_images[model] += n
            self._rate_win[model].append((now, n))
            bs = self.batchsize.get(model, n)
            if hit is not None:
                # c2 needs the chunk's dispatch time: a result that reaches the
                # standby before the replicated assignment has none (it would
                # enter the window as a 0-second chunk)
                self._ptime_win[model].append((now, (now - t_start) / n * bs))
            self._expire(model, now)
            self._c2_dirty.add(model)   # stats recomputed when read (c2 / snapshot), not per chunk
            self.results[f"{model} {qnum}"].append(
                ChunkResult(start, end, np.asarray(cls, dtype=np.int32), np.asarray(prob, dtype=np.float32),
                            worker))
            self._bump("result", model, qnum, start, end, now)
            return True

    def record_results(self, recs, now: float | None = None) -> int:
        """Ingest several finished chunks [(model, qnum, worker, s, e, cls,
        prob)] under one lock hold (a collective round); returns how many were
        new.  Same semantics as ``record_result`` per chunk.  The common case
        -- every chunk of the round is a fresh answer to a running chunk of
        one query -- is done in bulk: one pass over the query's entries, one
        interval merge, one window entry and ONE replication op; anything else
        (duplicates, re-split ranges, several queries) takes the per-chunk path."""
        now = self.clock() if now is None else now
        with self.lock:
            if recs and self._whole_ok(recs):
                return self._record_whole(recs, now)
            if recs and self._bulk_ok(recs):
                return self._record_bulk(recs, now)
            return sum(1 for m, q, w, s, e, c, p in recs if self.record_result(m, q, w, s, e, c, p, now))

    def _whole_ok(self, recs) -> bool:
        """The commonest round: it answers EVERY chunk of one query and nothing
        of that query is held yet (a query split over the round's members,
        VERDICT r5 item 6).  Then every entry is 'w' (the open count equals the
        entry count) and no chunk is a duplicate.  In any order: the round lists
        members in group order, the plan has the scheduler's sampled order."""
        model, qnum = recs[0][0], recs[0][1]
        key = (model, qnum)
        ents = self.worker_set.get(key)
        if not ents or len(ents) != len(recs) or self._open.get(key) != len(recs) or self._done_imgs.get(key):
            return False
        want = {(ent[0], ent[1], ent[2]) for ent in ents}
        for r in recs:
            if r[0] != model or r[1] != qnum or (r[2], r[3], r[4]) not in want:
                return False
        return len(want) == len(recs) == len({(r[2], r[3], r[4]) for r in recs})

    def _record_whole(self, recs, now: float) -> int:
        """``_record_bulk`` for a round that closes its whole query (``_whole_ok``):
        one pass in arrival order (the order per-chunk ``record_result`` would
        append results and times in), the entries rewritten in their own order,
        the query's done intervals set at once."""
        model, qnum = recs[0][0], recs[0][1]
        key = (model, qnum)
        ents = self.worker_set[key]
        bsz = self.batchsize.get(model)
        vms = self.working_vm_set
        done_add = self._done_keys.add
        pw_append = self._ptime_win[model].append
        res = self.results[f"{model} {qnum}"]
        i32, f32, nd = np.int32, np.float32, np.ndarray
        chunks, tot = [], 0
        t0s = {(x[0], x[1], x[2]): x[4] for x in ents}
        for r in recs:
            w, s, e = r[2], r[3], r[4]
            t_start = t0s[(w, s, e)]
            ck = (model, qnum, s, e)
            vm = vms.get(w)
            if vm is not None:
                if vm and vm[0] == ck:
                    del vm[0]
                else:
                    try:
                        vm.remove(ck)
                    except ValueError:
                        pass
                if not vm:
                    del vms[w]
            done_add(ck)
            n = e - s + 1
            tot += n
            pw_append((now, (now - t_start) * (1.0 if bsz is None else bsz / n)))
            c, p = r[5], r[6]
            res.append(ChunkResult(s, e, c if type(c) is nd and c.dtype == i32 else np.asarray(c, dtype=i32),
                                   p if type(p) is nd and p.dtype == f32 else np.asarray(p, dtype=f32), w))
            chunks.append([s, e])
        self.worker_set[key] = [(x[0], x[1], x[2], "f", x[4], now) for x in ents]
        self._open.pop(key, None)
        chunks.sort()
        ivs = self._done_imgs[key]
        cs, ce = chunks[0]
        for s, e in chunks[1:]:
            if s == ce + 1:
                ce = e
            else:
                _add_interval(ivs, cs, ce)
                cs, ce = s, e
        _add_interval(ivs, cs, ce)
        self.finished_queries[model] += 1
        t0 = self.query_submit_time.get(key)
        if t0 is not None:
            self.query_latency[model].append(now - t0)
        self.finished_images[model] += tot
        self._rate_win[model].append((now, tot))
        self._expire(model, now)
        self._c2_dirty.add(model)
        self._bump("results", model, qnum, chunks, now)
        return len(recs)

    def _bulk_ok(self, recs) -> bool:
        model, qnum = recs[0][0], recs[0][1]
        key = (model, qnum)
        if key not in self._open:
            return False
        running = {(x[0], x[1], x[2]) for x in self.worker_set.get(key, ()) if x[3] == "w"}
        done = self._done_keys
        rng = []
        for r in recs:
            if r[0] != model or r[1] != qnum:
                return False
            s, e = int(r[3]), int(r[4])
            if (r[2], s, e) not in running or (model, qnum, s, e) in done:
                return False
            rng.append((s, e))
        rng.sort()
        for a, b in zip(rng, rng[1:]):
            if a[1] >= b[0]:
                return False                               # overlapping chunks: per-chunk dedupe
        ivs = self._done_imgs.get(key)
        return not ivs or not any(a <= e and s <= b for s, e in rng for a, b in ivs)

    def _record_bulk(self, recs, now: float) -> int:
        model, qnum = recs[0][0], recs[0][1]
        key = (model, qnum)
        ents = self.worker_set[key]
        pos = {(x[0], x[1], x[2]): i for i, x in enumerate(ents) if x[3] == "w"}
        bsz = self.batchsize.get(model)             # None: per-chunk time, as record_result
        tot = 0
        res_append = self.results[f"{model} {qnum}"].append
        chunks = []
        vms = self.working_vm_set
        done_add = self._done_keys.add
        pw_append = self._ptime_win[model].append
        i32, f32, nd = np.int32, np.float32, np.ndarray
        for _, _, w, s, e, c, p in recs:
            i = pos[(w, s, e)]
            t_start = ents[i][4]
            ents[i] = (w, s, e, "f", t_start, now)
            ck = (model, qnum, s, e)
            vm = vms.get(w)
            if vm is not None:
                if vm and vm[0] == ck:                  # the usual case: the worker's oldest chunk
                    del vm[0]
                else:
                    try:
                        vm.remove(ck)
                    except ValueError:
                        pass
                if not vm:
                    del vms[w]
            done_add(ck)
            n = e - s + 1
            tot += n
            pw_append((now, (now - t_start) * (1.0 if bsz is None else bsz / n)))
            res_append(ChunkResult(s, e, c if type(c) is nd and c.dtype == i32 else np.asarray(c, dtype=i32),
                                   p if type(p) is nd and p.dtype == f32 else np.asarray(p, dtype=f32), w))
            chunks.append([s, e])
        self._open_add(key, -len(recs))
        # the round's chunks are usually one contiguous range: merge them first, then
        # into the query's done intervals once per run
        chunks.sort()
        ivs = self._done_imgs[key]
        cs, ce = chunks[0]
        for s, e in chunks[1:]:
            if s == ce + 1:
                ce = e
            else:
                _add_interval(ivs, cs, ce)
                cs, ce = s, e
        _add_interval(ivs, cs, ce)
        if key not in self._open:
            self.finished_queries[model] += 1
            t0 = self.query_submit_time.get(key)
            if t0 is not None:
                self.query_latency[model].append(now - t0)
        self.finished_images[model] += tot
        self._rate_win[model].append((now, tot))
        self._expire(model, now)
        self._c2_dirty.add(model)
        self._bump("results", model, qnum, chunks, now)
        return len(recs)

    def reopen_unheld(self) -> int:
        """Chunks marked finished in the replicated tables whose images this
        node never received (their RESULT reached only the old coordinator)
        go back to 'w', so a promoted standby recomputes them instead of
        reporting a query done whose results it cannot show (c4)."""
        with self.lock:
            return self._reopen_locked(emit=True)

    def _reopen_locked(self, emit: bool) -> int:
        n = 0
        for (m, q), ents in self.worker_set.items():
            ivs = self._done_imgs.get((m, q), [])
            for i, (w, s, e, st, t0, t1) in enumerate(ents):
                if st == "f" and not any(a <= s and e <= b for a, b in ivs):
                    ents[i] = (w, s, e, "w", t0, t1)
                    self.working_vm_set[w].append((m, q, s, e))
                    self._open_add((m, q), 1)
                    n += 1
        if n and emit:
            self._bump("reopen")
        return n

    def replan(self, model: str, qnum, old, new, now: float | None = None) -> bool:
        """Replace a queued query's chunk plan (not started anywhere yet) by
        ``new`` [(worker, s, e)]: the coordinator re-splits queries that wait
        in the round queue when a second job changes the fair-time partition.
        False (nothing changed) unless every old chunk is still 'w' as given."""
        now = self.clock() if now is None else now
        with self.lock:
            return self._replan_locked(model, qnum, old, new, now, emit=True)

    def _replan_locked(self, model, qnum, old, new, now, emit: bool) -> bool:
        key = (model, qnum)
        ents = self.worker_set.get(key, [])
        old = {(w, int(s), int(e)) for w, s, e in old}
        have = {(x[0], x[1], x[2]) for x in ents if x[3] == "w"}
        if not old or not old <= have:
            return False
        self.worker_set[key] = [x for x in ents if not (x[3] == "w" and (x[0], x[1], x[2]) in old)]
        for w, s, e in old:
            try:
                self.working_vm_set[w].remove((model, qnum, s, e))
            except ValueError:
                pass
            if not self.working_vm_set.get(w):
                self.working_vm_set.pop(w, None)
        self._open_add(key, -len(old))
        for w, s, e in new:
            self.worker_set[key].append((w, int(s), int(e), "w", now, now))
            self.working_vm_set[w].append((model, qnum, int(s), int(e)))
            self._open_add(key, 1)
        if emit:
            self._bump("replan", model, qnum, [list(c) for c in sorted(old)], [list(c) for c in new], now)
        return True

    def chunks_of(self, worker: str) -> list[tuple]:
        with self.lock:
            return list(self.working_vm_set.get(worker, []))

    def busy_workers(self) -> dict:
        """worker -> the models it has chunks running of (the fair-time
        hand-over waits for a worker's chunks of its old job)."""
        with self.lock:
            return {w: {c[0] for c in cs} for w, cs in self.working_vm_set.items() if cs}

    def reassign(self, failed: str, new_worker: str, chunk: tuple, now: float | None = None) -> None:
        """Move one in-flight chunk of a failed worker to ``new_worker``
        (reference transfer_failed_inference_work, mp4_machinelearning.py:706-760)."""
        now = self.clock() if now is None else now
        with self.lock:
            self._reassign_locked(failed, new_worker, tuple(chunk), now, emit=True)

    def _reassign_locked(self, failed, new_worker, chunk, now, emit: bool) -> None:
        model, qnum, s, e = chunk
        key = (model, qnum)
        ents = self.worker_set[key]
        for i, ent in enumerate(ents):
            if ent[0] == failed and ent[1] == s and ent[2] == e and ent[3] == "w":
                ents.pop(i)
                self._open_add(key, -1)
                break
        ents.append((new_worker, s, e, "w", now, now))
        self._open_add(key, 1)
        try:
            self.working_vm_set[failed].remove(chunk)
        except (ValueError, KeyError):
            pass
        if not self.working_vm_set.get(failed):
            self.working_vm_set.pop(failed, None)
        self.working_vm_set[new_worker].append(chunk)
        if emit:
            self._bump("reassign", failed, new_worker, list(chunk), now)

    def pending(self) -> list[tuple]:
        """All chunks still marked 'w': [(model, qnum, worker, s, e, t_start)]."""
        with self.lock:
            out = []
            for (model, q) in self._open:
                for w, s, e, st, t0, _ in self.worker_set.get((model, q), []):
                    if st == "w":
                        out.append((model, q, w, s, e, t0))
            return out

    def active_models(self) -> set:
        """Models with a chunk still running or a coordinator-side job not yet
        fully submitted: O(open queries + jobs), no copy of the chunk tables
        (the per-submit / per-round scheduler check).  A job counts as active
        from its submission to its last result, including the moments between
        two of its queries, so the other job's split does not flip to "alone"
        and back at every refill of its window."""
        with self.lock:
            act = {m for (m, _q) in self._open}
            act.update(j["model"] for j in self.jobs.values() if j["next"] <= j["end"])
            return act

    def pending_count(self) -> int:
        with self.lock:
            return sum(self._open.values())

    def open_queries(self, model: str, qlo: int, qhi: int) -> int:
        """Queries of ``model`` numbered in [qlo, qhi] that still have chunks
        running (a coordinator-side job's window, O(open queries))."""
        with self.lock:
            return sum(1 for (m, q) in self._open if m == model and isinstance(q, int) and qlo <= q <= qhi)

    # -- metrics ------------------------------------------------------------------
    def _expire(self, model: str, now: float) -> None:
        for win in (self._rate_win[model], self._ptime_win[model]):
            while win and now - win[0][0] > self.window_s:
                win.popleft()

    def _refresh_c2(self) -> None:
        """Recompute the c2 statistics of models that got results since the
        last read.  Ingest only marks them stale: a per-chunk O(window)
        percentile costs the coordinator ~0.1 ms per chunk, and on the 8-rank
        throughput path a 30 s window holds tens of thousands of chunks."""
        for m in list(self._c2_dirty):
            self._expire(m, self.clock())
            self._recompute_c2(m)
        self._c2_dirty.clear()

    def _recompute_c2(self, model: str) -> None:
        vals = [v for _, v in self._ptime_win[model]]
        if vals:
            a = np.asarray(vals, dtype=np.float64)
            self.query_processing_time_meta[model] = [float(a.mean()), float(np.percentile(a, 25)),
                                                      float(np.percentile(a, 50)),
                                                      float(np.percentile(a, 75)), float(a.std())]

    def images_done(self, model: str) -> int:
        with self.lock:
            return int(self.finished_images.get(model, 0))

    def summary(self) -> dict:
        """Consistent view for the ``summary`` stats request (one lock hold: the
        tables are appended to by the result-ingest threads meanwhile)."""
        with self.lock:
            return {"ok": True, "done": {m: self.images_done(m) for m in self.models()},
                    "pending": self.pending_count(),
                    "latency": {m: list(v) for m, v in self.query_latency.items()},
                    "finished_queries": dict(self.finished_queries)}

    def rates(self, model: str, now: float | None = None) -> dict:
        now = self.clock() if now is None else now
        with self.lock:
            self._expire(model, now)
            win = self._rate_win[model]
            imgs = sum(n for _, n in win)
            span = self.window_s
            if win:
                span = max(min(self.window_s, now - win[0][0]), 1e-9)
            ips = imgs / span if win else 0.0
            return {"images_per_s": ips, "queries_per_s": ips / self.batchsize.get(model, 1),
                    "finished_images": self.images_done(model),
                    "finished_queries": int(self.finished_queries.get(model, 0))}

    def models(self) -> list[str]:
        with self.lock:
            ms = set(self.finished_images) | {m for m, _ in self.worker_set}
            return sorted(ms) or ["resnet18", "alexnet"]

    # -- shell views ------------------------------------------------------------
    def c1(self) -> str:
        """Query rate + finished count per model, reference labels (:1257-1267)."""
        label = {"resnet18": "Resnet18", "alexnet": "AlexNet"}
        lines = []
        for m in self.models():
            r = self.rates(m)
            L = label.get(m, m)
            lines.append(f"{L} query rate is {r['images_per_s']}")
            lines.append(f"{L} finished inference is {r['finished_images']}")
            lines.append(f"{L} finished batchsize query rare is {r['queries_per_s']}")
        return "\n".join(lines)

    def c2(self) -> str:
        """Processing-time stats per model over the sliding window (:1232-1253)."""
        lines = []
        with self.lock:
            self._refresh_c2()
            for m, v in sorted(self.query_processing_time_meta.items()):
                lines += [f"model {m} processing time", f"average {v[0]}", f"q1 {v[1]}", f"q2 {v[2]}",
                          f"q3 {v[3]}", f"stddev {v[4]}"]
        return "\n".join(lines)

    def inference_result_list(self) -> dict:
        names = self.names or class_names()
        with self.lock:
            return {k: [c.render(names) for c in sorted(v, key=lambda c: c.start)]
                    for k, v in self.results.items()}

    def c4(self, path: str = "result.txt") -> str:
        d = self.inference_result_list()
        with open(path, "w") as f:
            f.write(json.dumps(d))
        return str(d)

    def cq(self) -> str:
        with self.lock:
            return str(dict(self.worker_set))

    def cvm(self) -> str:
        with self.lock:
            return str(dict(self.working_vm_set))

    # -- replication (hot standby) --------------------------------------------------
    def snapshot(self, include_results: bool = True) -> dict:
        """Structured, JSON/msgpack-able snapshot (fix A12: no raw str() dumps).

        The coordinator's periodic push to the standby omits results: workers
        send every RESULT to the standby directly."""
        with self.lock:
            self._refresh_c2()
            return {
                "seq": self.seq,
                "worker_set": [[list(k), [list(e) for e in v]] for k, v in self.worker_set.items()],
                "working_vm_set": {w: [list(c) for c in v] for w, v in self.working_vm_set.items()},
                "results": ({k: [[c.start, c.end, c.cls.tolist(), c.prob.tolist(), c.worker] for c in v]
                             for k, v in self.results.items()} if include_results else None),
                "finished_images": dict(self.finished_images),
                "finished_queries": dict(self.finished_queries),
                "next_qnum": dict(self.next_qnum),
                "meta": dict(self.query_processing_time_meta),
                "submit": [[list(k), t] for k, t in self.query_submit_time.items()],
                "jobs": [[j, v] for j, v in self.jobs.items()],
            }

    def restore(self, snap: dict, keep_results: bool = False) -> None:
        """Adopt a snapshot.  With ``keep_results`` (standby mirror) the locally
        received results and counters are kept and chunks already answered
        stay marked 'f' even if the snapshot predates their RESULT."""
        with self.lock:
            if snap["seq"] < self.seq and not keep_results:
                return
            self.seq = max(self.seq, snap["seq"])
            self._log, self._log_base = [], self.seq      # history before the snapshot is not in the log
            self.worker_set = defaultdict(list)
            for k, v in snap["worker_set"]:
                self.worker_set[(k[0], k[1])] = [tuple(e) for e in v]
            self.working_vm_set = defaultdict(list, {w: [tuple(c) for c in v]
                                                     for w, v in snap["working_vm_set"].items()})
            if snap.get("results") is not None:
                self.results = defaultdict(list)
                self._done_keys = set()
                self._done_imgs = defaultdict(list)
                for k, v in snap["results"].items():
                    model, q = k.rsplit(" ", 1)
                    qn = int(q) if q.lstrip("-").isdigit() else q
                    for s, e, c, p, w in v:
                        self.results[k].append(ChunkResult(s, e, np.asarray(c, np.int32),
                                                           np.asarray(p, np.float32), w))
                        self._done_keys.add((model, qn, s, e))
                        _add_interval(self._done_imgs[(model, qn)], s, e)
            if not keep_results:
                self.finished_images = defaultdict(int, snap["finished_images"])
                self.finished_queries = defaultdict(int, snap["finished_queries"])
            # reconcile: chunks we already hold a result for are finished
            for (model, q), ents in self.worker_set.items():
                for i, (w, s, e, st, t0, t1) in enumerate(ents):
                    if st == "w" and (model, q, s, e) in self._done_keys:
                        ents[i] = (w, s, e, "f", t0, t1)
                        try:
                            self.working_vm_set[w].remove((model, q, s, e))
                        except ValueError:
                            pass
            for w in [w for w, v in self.working_vm_set.items() if not v]:
                self.working_vm_set.pop(w)
            self._open = {}
            self._spans = set()
            for key, ents in self.worker_set.items():
                nw = sum(1 for ent in ents if ent[3] == "w")
                if nw:
                    self._open[key] = nw
                if ents:
                    self._spans.add((key[0], min(x[1] for x in ents), max(x[2] for x in ents)))
            if keep_results:
                self.mirror_seq = int(snap["seq"])        # deltas continue from the snapshot
            for m, n in snap["next_qnum"].items():
                self.next_qnum[m] = max(self.next_qnum.get(m, 0), n)
            self.query_processing_time_meta.update(snap["meta"])
            for k, t in snap.get("submit", []):
                self.query_submit_time.setdefault((k[0], k[1]), t)
            for j, v in snap.get("jobs", []):
                cur = self.jobs.get(j)
                if cur is None or v["next"] > cur["next"]:
                    self.jobs[j] = dict(v)
            racecheck.instrument(self, self._TABLES)
