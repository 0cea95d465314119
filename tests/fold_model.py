"""A numpy model of the R2 key-log fold (include/sbmp/r2_fold.h states the rule; this shares no
code with it): the slot index by arange, two masks, and one np.bincount in int64 per kind and
iteration.  Integer counts: no tolerance anywhere.

fold_model(..., alter=NAME) is a deliberately wrong fold, one per entry of ALTERATIONS; the CPU
tests show that each differs from the host twin on the cases named there, so a kernel wrong in
that way cannot pass.
"""
import numpy as np

BLOCK = 256   # slots per block, the unit dealt round-robin to ranks (the rule's, not a tunable)

# alteration -> the cases (tests/fold_cases.py) on which it must change a count
ALTERATIONS = {
    "no-S-mask": ("S-1024-at-257", "window-40-64", "window-0-64"),
    "slot<=S": ("S-1024-at-0", "S-big-at-per", "ranks-P3-r1"),
    "mask-by-8-keys": ("S-1024-at-1", "S-1024-at-7", "S-1024-at-9", "S-big-at-per+1", "window-0-64"),
    "no-executed-test": ("window-31-64-holes", "window-none-executed"),
    "row-t+1": ("window-0-1", "window-40-64", "window-127-1"),
    "row-t-no-modulo": ("window-40-64", "window-127-1"),
    "rank-term-dropped": ("ranks-P2-r1", "ranks-P3-r2", "ranks-P8-r7"),
    "stride-on-rank": ("ranks-P2-r1", "ranks-P3-r1", "ranks-P8-r3"),
    "wrap-16-bit": ("counter-two-iterations",),
    "0x7fff-is-a-cell": ("dropped-keys",),
    "tables-overwritten": ("counter-valid-cell0-prior7", "counter-half-cellmax-priorbig"),
}


def fold_model(ring, S, executed, tFirst, nR2, *, rank=0, nranks=1, R2Valid=None, R2Invalid=None, alter=None):
    """ring (window, logSlots) uint16; S, executed: one entry per iteration from tFirst on.
    Returns (R2Valid, R2Invalid) as int64 arrays: the prior contents plus the counts."""
    assert alter is None or alter in ALTERATIONS, alter
    ring = np.asarray(ring)
    window, logSlots = ring.shape
    i = np.arange(logSlots, dtype=np.int64)
    slot = (rank + nranks * (i // BLOCK)) * BLOCK + i % BLOCK
    if alter == "rank-term-dropped":
        slot = (nranks * (i // BLOCK)) * BLOCK + i % BLOCK
    elif alter == "stride-on-rank":
        slot = (nranks * rank + i // BLOCK) * BLOCK + i % BLOCK
    counts = [np.zeros(nR2, dtype=np.int64), np.zeros(nR2, dtype=np.int64)]   # invalid, valid
    for j, (s, ex) in enumerate(zip(np.asarray(S).tolist(), np.asarray(executed).tolist())):
        t = tFirst + j
        if not ex and alter != "no-executed-test":
            continue
        r = t % window
        if alter == "row-t+1":
            r = (t + 1) % window
        if alter == "row-t-no-modulo":   # past the ring: nothing a fold may count lies there
            key = ring[t].astype(np.int64) if t < window else np.full(logSlots, 0xffff, dtype=np.int64)
        else:
            key = ring[r].astype(np.int64)
        cell = key & 0x7fff
        below = slot < s
        if alter == "no-S-mask":
            below = np.ones(logSlots, dtype=bool)
        elif alter == "slot<=S":
            below = slot <= s
        elif alter == "mask-by-8-keys":   # a whole 8-key piece lives or dies with its first slot
            below = (slot // 8) * 8 < s
        ingrid = cell < nR2
        if alter == "0x7fff-is-a-cell":   # only the planner's own 0xffff is dropped
            ingrid = key != 0xffff
            cell = cell % nR2
        live = below & ingrid
        for kind in (0, 1):
            counts[kind] += np.bincount(cell[live & ((key >> 15) == kind)], minlength=nR2)
    if alter == "wrap-16-bit":
        counts = [c & 0xffff for c in counts]
    prior = [np.zeros(nR2, dtype=np.int64) if p is None else np.asarray(p, dtype=np.int64) for p in (R2Valid, R2Invalid)]
    if alter == "tables-overwritten":
        prior = [np.where(c > 0, 0, p) for c, p in zip((counts[1], counts[0]), prior)]
    return prior[0] + counts[1], prior[1] + counts[0]
