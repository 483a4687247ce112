"""What a MIC2 crop call with a frame cache does, written from its text in include/mic_hip.h (no test in here): the host model that
tests/test_mic2_frame_cache_cpu.py pins by hand-worked traces and tests/test_gpu_mic2_frame_cache.py holds the device path against.

One cache, any number of readers.  files[r] = (nframes, temporal) of reader r.  A call is a list of (reader, named frames) in the
order of the readers' array, each reader once; its keys are the named frames ascending, reader after reader.  The replacement
policy is tile_cache_model.lru_model's; the model walks it call by call (a call may release entries, which a whole-trace function
cannot be told), and predict() checks every failure-free prefix of a trace against lru_model itself."""
from tile_cache_model import lru_model

HIT, MISS, BYPASS = 0, 1, 2


def key(reader, frame):
    """the key as mic_hip_tile_cache_plan takes it: ascending over a call's (reader, frame) pairs"""
    return (reader << 32) | frame


def keys_of(call):
    return [key(r, f) for r, frames in call for f in sorted(set(frames))]


class FrameCacheModel:
    def __init__(self, nslots, files):
        self.files = list(files)
        self.slots = [None] * nslots            # (key, stamp)
        self.number = 0
        self.counters = dict(hits=0, misses=0, bypassed=0, evictions=0, calls=0)
        self._trace, self._clean = [], True     # the keys of every call so far; no call has released or failed yet

    def resident(self):
        return {e[0] for e in self.slots if e is not None}

    def _plan(self, keys):
        """lru_model's steps (1) and (2) for one call on the model's own slots"""
        self.number += 1
        number, slots = self.number, self.slots
        out = [None] * len(keys)
        where = {e[0]: q for q, e in enumerate(slots) if e is not None}
        for i, k in enumerate(keys):
            if k in where:
                slots[where[k]] = (k, number)
                out[i] = HIT
        evictions = 0
        for i, k in enumerate(keys):
            if out[i] is not None:
                continue
            free = [q for q, e in enumerate(slots) if e is None]
            if free:
                q = free[0]
            else:
                old = [(e[1], q) for q, e in enumerate(slots) if e[1] < number]
                if not old:
                    out[i] = BYPASS
                    continue
                q = min(old)[1]
                evictions += 1
            slots[q] = (k, number)
            out[i] = MISS
        return out, evictions

    def call(self, call, bad=()):
        """call: [(reader, frames)]; bad: (reader, frame) pairs whose stream fails to decode.
        -> dict(outcomes = {(reader, frame): HIT / MISS / BYPASS}, anchors = {(reader, frame): anchor frame or None} for the non-hit
        named frames of temporal readers, decoded = the set of (reader, frame) streams entropy-decoded, failed = {(reader, frame):
        the failing frame} for the named frames that are lost, resident = the keys resident afterwards)"""
        bad = set(bad)
        keys = keys_of(call)
        out, evictions = self._plan(keys)
        outcomes = {(k >> 32, k & 0xFFFFFFFF): o for k, o in zip(keys, out)}
        c = self.counters
        c["calls"] += 1
        c["evictions"] += evictions
        for o in out:
            c[("hits", "misses", "bypassed")[o]] += 1
        after_plan = self.resident()
        anchors, decoded, failed = {}, set(), {}
        for r, frames in call:
            named = sorted(set(frames))
            need = [f for f in named if outcomes[(r, f)] != HIT]
            if not self.files[r][1]:
                decoded |= {(r, f) for f in need}
                failed.update({(r, f): f for f in need if (r, f) in bad})
                continue
            mine = sorted(k & 0xFFFFFFFF for k in after_plan if k >> 32 == r)
            streams = set()
            for f in need:
                below = [a for a in mine if a < f]
                a = below[-1] if below else None
                anchors[(r, f)] = a
                streams |= set(range(0 if a is None else a + 1, f + 1))
            decoded |= {(r, g) for g in streams}
            # a run is a stretch of consecutive decoded frames; it is lost from its first failing stream on
            dead = None
            for g in sorted(streams):
                if g - 1 not in streams:
                    dead = None
                if dead is None and (r, g) in bad:
                    dead = g
                if dead is not None and g in named:
                    failed[(r, g)] = dead
        for (r, f) in failed:                   # a lost frame is never resident: released, it counts as bypassed
            if outcomes[(r, f)] == MISS:
                q = [q for q, e in enumerate(self.slots) if e is not None and e[0] == key(r, f)][0]
                self.slots[q] = None
                c["misses"] -= 1
                c["bypassed"] += 1
        self._trace.append(keys)
        self._clean = self._clean and not failed
        if self._clean:                         # the whole-trace model says the same
            outs, ev, res = lru_model(len(self.slots), self._trace)
            assert outs[-1] == out and ev == c["evictions"] and res[-1] == self.resident()
        return dict(outcomes=outcomes, anchors=anchors, decoded=decoded, failed=failed, resident=self.resident())

    def clear(self):
        self.slots = [None] * len(self.slots)
        self._clean = False                     # (lru_model knows no clear)


def predict(nslots, files, calls, bad=None):
    """the model over a trace: calls[k] as FrameCacheModel.call takes it, bad[k] the failing streams of call k -> (results, counters)"""
    m = FrameCacheModel(nslots, files)
    res = [m.call(c, (bad or {}).get(k, ())) for k, c in enumerate(calls)]
    return res, dict(m.counters)
