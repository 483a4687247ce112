"""The replacement policy of the MIC3 tile cache, written from its text in include/mic_hip.h (no test in here): the host model that
tests/test_tile_cache_cpu.py holds mic_hip_tile_cache_plan against and tests/test_gpu_wsi_tile_cache.py the device path."""


def lru_model(nslots, calls):
    """Each call gets the next call number.  (1) Its keys are walked in order; a resident one is a hit and is stamped with the call
    number.  (2) Each miss, in order, takes the lowest-numbered free slot; else the entry with the smallest stamp below the call's
    number, ties to the lowest slot, which is evicted; else it is bypassed.
    -> (outcomes per call: 0 hit, 1 miss, 2 bypassed; evictions in all; residency (set of keys) after each call)"""
    slots = [None] * nslots                 # (key, stamp)
    outs, evictions, resident = [], 0, []
    for number, keys in enumerate(calls, start=1):
        out = [None] * len(keys)
        where = {e[0]: q for q, e in enumerate(slots) if e is not None}
        for i, k in enumerate(keys):
            if k in where:
                slots[where[k]] = (k, number)
                out[i] = 0
        for i, k in enumerate(keys):
            if out[i] is not None:
                continue
            free = [q for q, e in enumerate(slots) if e is None]
            if free:
                q = free[0]
            else:
                old = [(e[1], q) for q, e in enumerate(slots) if e[1] < number]
                if not old:
                    out[i] = 2
                    continue
                q = min(old)[1]
                evictions += 1
            slots[q] = (k, number)
            out[i] = 1
        outs.append(out)
        resident.append({e[0] for e in slots if e is not None})
    return outs, evictions, resident
