"""Specification of unsegment (Glu) and shuffle (Shf) (TEST INFRASTRUCTURE ONLY).

  * `glue_spec` / `shuffle_spec`: the two modules as sequential loops over the molecules of oracle/mdf_ops_oracle.py (stream_mdf with
    unroll=True / write_mdf), with the build's counter-based draws (Philox keyed by (seed, molecule index, stream, block)); the HIP
    kernels (tksm_amd/csrc/mdf_kernels.hip) reproduce them bit for bit, without the loops.
  * `shuffle_reference`: Shuffle_module::shuffle_stream (src/shuffle.cpp:23-44) line by line with numpy's generator standing in for
    mt19937 -- for checking distributions.
Two departures from Unsegment_module::run (src/unsegment.cpp:88-105) are part of the definition: the last chain is written (the
reference never writes its last `current`), and every unrolled molecule draws for itself (the reference glues records)."""
import copy

import numpy as np

from core_modules_spec import philox_np

ST_GLUE, ST_SHF_KEY, ST_SHF_SLOT = 30, 31, 35


def joins_np(seed, p, g):
    """joins(g) over an array of molecule indices: g > 0 and u01(philox(seed, g, ST_GLUE, 0).x) < p (NaN: never)"""
    g = np.asarray(g, np.uint64)
    u = philox_np(seed, g, ST_GLUE, 0)[0].astype(np.float64) * (1.0 / 4294967296.0)
    return (g > 0) & (u < p)


def glue_spec(mols, p, seed, first=0):
    """molecule i joins the chain before it iff i > 0 and joins(first + i); a chain is the head with the joiners' segments behind its
    own and their written ids under Cat (molecule_descriptor::concat, add_comment: src/interval.h:893-896, src/unsegment.cpp:99)"""
    j = joins_np(seed, p, first + np.arange(len(mols), dtype=np.uint64)) if mols else []
    out, cur = [], None
    for i, md in enumerate(mols):
        if cur is not None and j[i]:
            cur["segments"] += copy.deepcopy(md["segments"])
            cur["meta"].setdefault("Cat", []).append(md["id"])
        else:
            if cur is not None:
                out.append(cur)
            cur = copy.deepcopy(md)
            cur["depth"] = 1
    if cur is not None:
        out.append(cur)                                                # (the reference stops without this line)
    return out


def chains(n, p, seed, first=0):
    """the lengths of the chains glue_spec makes of n molecules"""
    heads = np.flatnonzero(~joins_np(seed, p, first + np.arange(n, dtype=np.uint64)) | (np.arange(n) == 0))
    return np.diff(np.append(heads, n))


def shuffle_draws(n, seeds, B=0):
    """the draws of a run for every seed of `seeds` (an array): slots [len(seeds), n - B] = umulhi(philox(seed, t, ST_SHF_SLOT, 0).x, B) for
    t = B .. n-1, keys [len(seeds), B] = x << 32 | y of philox(seed, s, ST_SHF_KEY, 0) for the slots s"""
    if B == 0 or B >= n:
        B = n
    seeds = np.asarray(seeds, np.uint64).reshape(-1, 1)
    t = np.broadcast_to(np.arange(B, n, dtype=np.uint64), (len(seeds), n - B))
    s = np.broadcast_to(np.arange(B, dtype=np.uint64), (len(seeds), B))
    slots = (philox_np(seeds, t, ST_SHF_SLOT, 0)[0] * np.uint64(B)) >> np.uint64(32) if n > B else np.zeros((len(seeds), 0), np.uint64)
    w = philox_np(seeds, s, ST_SHF_KEY, 0) if B else (s, s)
    return slots, (w[0] << np.uint64(32)) | w[1]


def shuffle_order(n, seed, B=0, draws=None):
    """the input index of every output molecule: the buffer loop, literally.  draws: this seed's rows of shuffle_draws (made here if None)"""
    if B == 0 or B >= n:
        B = n
    slots, keys = draws if draws is not None else [x[0] for x in shuffle_draws(n, [seed], B)]
    slots, keys = [int(x) for x in slots], [int(x) for x in keys]
    buf, out = list(range(B)), []
    for k, slot in enumerate(slots):
        out.append(buf[slot])
        buf[slot] = B + k
    for s in sorted(range(B), key=lambda s: (keys[s], s)):
        out.append(buf[s])
    return out


def shuffle_spec(mols, seed, B=0):
    out = [copy.deepcopy(mols[i]) for i in shuffle_order(len(mols), seed, B)]
    for md in out:
        md["depth"] = 1
    return out


def shuffle_reference(n, B, rs):
    """shuffle_stream (src/shuffle.cpp:23-44) on molecules 0 .. n-1 with numpy's generator `rs`; B None: no --buffer-size"""
    buf, out = [], []
    for md in range(n):
        if B is None or B > len(buf):
            buf.append(md)
        else:
            pos = int(rs.randint(0, B))                                # uniform_int_distribution(0, buffer_size - 1)
            out.append(buf[pos])
            buf[pos] = md
    rs.shuffle(buf)
    return out + buf
