# -*- coding: utf-8 -*-
"""The staging layout of the host entry points (celerite2_amd/csrc/c2_host.hip), restated for the tests that need to know
where in the per-thread device arena an argument of a c2h_* call lands (tests/test_gpu_host_staging.py).

What it restates (line numbers of c2_host.hip as of this file's writing):
  * Staging::map (113-126) -- arguments that start at the same host address share one entry, which takes the longest
    length, is in/out as soon as one of them is written and stays `fresh` only while all of them are;
  * Staging::up (134) and kAlign (83) -- every entry is rounded up to 256 bytes (an empty one counts as 8 bytes);
  * Staging::commit (136-147) -- pure inputs in front, in/out arrays behind them, fresh outputs last, each group in
    registration order; the upload is [0, in + io), the fresh outputs occupy [in + io, total) and are never uploaded;
  * kBounceMax = 64 MiB (84; beyond it the arguments go up one by one: the direct path) and Arena::kKeepMax = 256 MiB
    (53; beyond it the arena is given back when the call returns);
  * the registration order of every c2h_* entry point (ORDER below: the st.in / st.out / st.fresh lines of each function,
    191-305; c2h_factor also stages its two-word pivot flag as an in/out entry).
Only poison() touches the device (through `driver`, imported when it is called)."""
import numpy as np

ALIGN = 256
BOUNCE_MAX = 64 << 20
KEEP_MAX = 256 << 20

IN, INOUT, FRESH = "in", "inout", "fresh"


def up(nbytes):
    return (max(int(nbytes), 8) + ALIGN - 1) // ALIGN * ALIGN


def layout(entries):
    """entries: the (host pointer, bytes, kind) of a call in registration order, kind one of IN / INOUT / FRESH (the
    pointer may be any hashable key).  Returns a dict: `offsets` (one per entry given, shared where the pointers are),
    `upload` (bytes [0, upload) go up), `fresh` (bytes [upload, total) are never uploaded), `total`."""
    merged, index = [], {}
    for ptr, nbytes, kind in entries:
        assert kind in (IN, INOUT, FRESH), kind
        if ptr in index:
            e = merged[index[ptr]]
            e["bytes"] = max(e["bytes"], int(nbytes))
            e["out"] = e["out"] or kind != IN
            e["fresh"] = e["fresh"] and kind == FRESH
        else:
            index[ptr] = len(merged)
            merged.append(dict(bytes=int(nbytes), out=kind != IN, fresh=kind == FRESH, off=None))
    off = 0
    for group in (lambda e: not e["out"], lambda e: e["out"] and not e["fresh"], lambda e: e["fresh"]):
        for e in merged:
            if group(e):
                e["off"] = off
                off += up(e["bytes"])
    upload = sum(up(e["bytes"]) for e in merged if not e["fresh"])
    return dict(offsets=[merged[index[ptr]]["off"] for ptr, _, _ in entries], upload=upload, fresh=off - upload, total=off)


# name -> ((argument, kind), ...) in the order c2_host.hip registers them ("flag": the entry c2h_factor adds itself)
ORDER = {
    "factor": (("t", IN), ("c", IN), ("a", IN), ("U", IN), ("V", IN), ("d", INOUT), ("W", INOUT), ("S", FRESH),
               ("flag", INOUT)),
    "sweep": (("t", IN), ("c", IN), ("U", IN), ("W", IN), ("Y", IN), ("Z", INOUT), ("F", FRESH)),
    "general": (("t1", IN), ("t2", IN), ("c", IN), ("U", IN), ("V", IN), ("Y", IN), ("Z", INOUT), ("F", INOUT)),
    "factor_rev": (("t", IN), ("c", IN), ("a", IN), ("U", IN), ("V", IN), ("d", IN), ("W", IN), ("S", IN), ("bd", IN),
                   ("bW", IN), ("bt", FRESH), ("bc", FRESH), ("ba", FRESH), ("bU", FRESH), ("bV", FRESH)),
    "sweep_rev": (("t", IN), ("c", IN), ("U", IN), ("W", IN), ("Y", IN), ("Z", IN), ("F", IN), ("bZ", IN), ("bt", FRESH),
                  ("bc", FRESH), ("bU", FRESH), ("bW", FRESH), ("bY", FRESH)),
    "get_celerite_matrices": (("ar", IN), ("ac", IN), ("bc", IN), ("dc", IN), ("x", IN), ("diag", IN), ("a", FRESH),
                              ("U", FRESH), ("V", FRESH)),
}


def entries(op, *arrays):
    """The entries of one call of `op` (a key of ORDER) on numpy arrays given in ORDER's order.  None stands for an
    argument the call leaves out (S or F of the driver forms); an empty array is left out as c2_host.hip leaves out the
    coefficient arrays of an absent term kind; the pivot flag of factor needs no array."""
    names = [n for n, _ in ORDER[op] if n != "flag"]
    assert len(arrays) == len(names), (op, len(arrays), names)
    given = dict(zip(names, arrays))
    out = []
    for name, kind in ORDER[op]:
        if name == "flag":
            out.append((("flag",), 8, kind))
            continue
        x = given[name]
        if x is None or x.size == 0:
            continue
        assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous, name
        out.append((x.ctypes.data, x.nbytes, kind))
    return out


def image(call_entries, arrays):
    """The float64 words of the upload [0, upload) a call makes: every uploaded array at its offset, NaN-free zeros in the
    padding between them (what the padding holds is not defined; zero is the pessimistic choice for a test that wants NaN).
    `arrays`: the arrays of `call_entries` that are not None / empty, in the same order."""
    lay = layout(call_entries)
    img = np.zeros(lay["upload"] // 8)
    assert len(arrays) == len(call_entries)
    for (_, nbytes, kind), off, x in zip(call_entries, lay["offsets"], arrays):
        if kind != FRESH and off + nbytes <= lay["upload"]:
            img[off // 8: (off + nbytes) // 8] = np.asarray(x, dtype=np.float64).ravel()
    return img


def _poison_call(upload_extent, total):
    """(function name, arguments, entries) of the smallest ordinary call whose uploaded NaN cover [upload_extent, total)."""
    nan = np.nan
    if upload_extent >= 4 * ALIGN:
        # driver.solve_lower, J = 1: t, c, U, W finite and in front; Y and Z (uploaded: Z is in/out) all NaN.  N * nrhs a
        # multiple of 32 makes Y a whole number of 256-byte units, so Y and Z are one NaN run with no padding between
        for N in range(1, 1 << 22):
            off_y = 3 * up(8 * N) + ALIGN
            if off_y > upload_extent:
                break
            for nrhs in range(1, 65):
                if (N * nrhs) % 32 == 0 and off_y + 16 * N * nrhs >= total:
                    t, c = np.arange(N, dtype=np.float64), np.ones(1)
                    U, W = np.zeros((N, 1)), np.zeros((N, 1))
                    Y, Z = np.full((N, nrhs), nan), np.full((N, nrhs), nan)
                    args = [t, c, U, W, Y, Z]
                    return "solve_lower", args, entries("sweep", *args, None)
        raise AssertionError("no solve_lower poison covers [%d, %d)" % (upload_extent, total))
    # a target with fewer than four arrays in front of its outputs (get_celerite_matrices of one real term): the same op
    # with 32 complex terms and every input NaN -- three coefficient arrays of 256 bytes, then x and diag, one NaN run from 0
    N = 32 * max(1, -(-(total - 3 * ALIGN) // (16 * 32)))
    ac, bc, dc = (np.full(32, nan) for _ in range(3))
    x, diag = np.full(N, nan), np.full(N, nan)
    args = [np.empty(0), ac, bc, dc, x, diag, np.empty(N), np.empty((N, 64)), np.empty((N, 64))]
    return "get_celerite_matrices", args, entries("get_celerite_matrices", *args)


def poison(upload_extent, total):
    """One ordinary drop-in call on the calling thread that leaves NaN on every byte of [upload_extent, total) of its
    staging arena: the region a following call with that upload extent and that total keeps for its never-uploaded
    outputs.  The NaN are UPLOADED (inputs and in/out arrays of the poisoning call), so where they lie follows from the
    layout alone, which is asserted here on the host before the call; the poisoning call's own total is at least `total`,
    so the arena is not reallocated between the two calls."""
    from celerite2_amd import driver

    assert 0 < upload_extent <= total and upload_extent % ALIGN == 0 and total % ALIGN == 0
    name, args, ents = _poison_call(upload_extent, total)
    lay = layout(ents)
    assert lay["total"] >= total, (lay, total)
    img = image(ents, [a for a in args if a.size])
    assert lay["upload"] >= total and np.isnan(img[upload_extent // 8: total // 8]).all(), (name, lay, upload_extent, total)
    getattr(driver, name)(*args)
