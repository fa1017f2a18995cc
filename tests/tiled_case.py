"""Tiled batches (test infrastructure for tests/test_gpu_batch_sizes.py): a few base problems copied
into a batch of any size, so that every element of a large batch has an exact expected value.

An element's result does not depend on its batch, its slot or its sweep partner, bit for bit
(tests/test_gpu_elements.py).  So: solve n base problems in a handle of their own
and check them against the oracle; fill a batch of B elements with copies of them (`tile`, by an
index map from `draw` / `draws`); every copy must then equal its base element exactly (`same`).

What `same` compares are the elements' records (Solver.export_elements: the compact route — the
gain rows stay compact, 12 x 24 per knot, where trajectory() expands them to 24 x 24), fetched in
chunks.  A record is the header and then the device rows of the element (hsddp_elements.h:
record_layout, restated in `record_fields` and checked against the library's record size and, on
the base handle, against what the download calls return).  Compared, byte for byte: the nominal and
working state and control rows, Defect, dX, dU, du, the compact gains, the reference rows, the slot
sums, the ReB pairs, the touchdown masks with their AL parameters and stored foot heights, the
contact rows, x0, the buffer selector, ElemState (cost, feasibility, merit, regularisation,
iteration and trial counts, status, the flags) and the solver-info history — every field
tests/restart_case.py's snapshot / same_element reads, and the ones behind them.

Excluded, and why:
  * the record header (version word, compatibility key, host bookkeeping).  The key describes the
    handle (S_cap, hashes of its weights and table), and the bookkeeping holds the element's layout,
    reach flags and contact rows as the *host* keeps them: those are compared through
    element_layouts() instead, and the contact rows are in the payload too;
  * rows past an element's own state slots and phases (padding at the handle's strides);
  * the stored GRF forces and their flags (cf_u, cf_flag) of an element whose ElemState::ovr is 0:
    hsddp_internal.h declares their contents arbitrary then, and nothing reads them.
"""
import numpy as np

NX, KCW, MAXP, MTD, REC_HIST = 24, 12 * 24, 16, 4, 256

ELEM_STATE = np.dtype([(k, np.float64) for k in ("cost", "feas", "merit", "merit_rho", "dV1", "dV2", "reg", "max_t", "max_p",
                                                  "max_t_prev", "max_p_prev", "cost_prev", "merit_prev", "feas_prev")] +
                      [(k, np.int32) for k in ("done", "inner_done", "ls_active", "accepted", "status", "iters", "outer_iters",
                                               "n_ls", "hist_n", "ovr", "td_stale", "inner_n")])
assert ELEM_STATE.itemsize == 160


# ---- index maps ----------------------------------------------------------------------------------------
def _groups(n, groups):
    g = [list(range(n))] if groups is None else [list(x) for x in groups]
    assert sorted(sum(g, [])) == list(range(n)), "groups must partition the base elements"
    return g


def sweep_pairs(index, groups=None, n=None):
    """The sweep's element pairs of a tiled batch as (first half-wave, second half-wave or -1): elements
    2q and 2q + 1 of a batch with one layout; with per-element layouts (`groups`: the base elements
    of each layout) consecutive elements of one layout, the layouts one after the other
    (hsddp_phases.h: pair_layouts)."""
    index = np.asarray(index)
    n = int(index.max()) + 1 if n is None else n
    out = []
    for g in _groups(n, groups):
        el = np.flatnonzero(np.isin(index, g))
        out += [(int(el[q]), int(el[q + 1]) if q + 1 < len(el) else -1) for q in range(0, len(el), 2)]
    return out


def n_pairs(index, groups=None, n=None):
    return len(sweep_pairs(index, groups, n))


def pairs_needed(n, groups=None):
    """batch size from which one map holds every ordered pair of sweep partners, element B - 1 chosen
    freely behind them and (several layouts: the pairs alone do not place them) room for every base
    element at every residue of b mod 4"""
    return 2 * sum(len(g) ** 2 for g in _groups(n, groups)) + 2 + (0 if groups is None else 4 * n + 3)


def coverage(maps, n, groups=None):
    """What the maps (index arrays of one batch size) cover together: the residues b mod 4 each base
    element takes, the base elements at B - 1 or beside it in the last pair, the ordered pairs of
    sweep partners."""
    res = [set() for _ in range(n)]
    last, pairs = set(), set()
    for index in maps:
        index = np.asarray(index)
        B = len(index)
        for b in range(B):
            res[index[b]].add(b % 4)
        for a, c in sweep_pairs(index, groups, n):
            if c >= 0:
                pairs.add((int(index[a]), int(index[c])))
            if B - 1 in (a, c):
                last |= {int(index[a])} | ({int(index[c])} if c >= 0 else set())
    return res, last, pairs


def assert_residues(maps, n):
    """every base element at every residue of b mod 4 (and so of b mod 2) that the batch size has"""
    B = len(maps[0])
    want = {b % 4 for b in range(B)}
    res, _, _ = coverage(maps, n)
    for i in range(n):
        assert res[i] == want, f"base element {i} only at residues {sorted(res[i])} mod 4 of {sorted(want)} (n = {n}, B = {B})"


def assert_pairs(maps, n, groups=None):
    """every ordered pair (base i, base j) of one layout as (first, second) half-wave of a sweep pair"""
    _, _, pairs = coverage(maps, n, groups)
    want = {(i, j) for g in _groups(n, groups) for i in g for j in g}
    assert want <= pairs, f"sweep pairs never formed: {sorted(want - pairs)} (n = {n}, B = {len(maps[0])})"


def assert_last(maps, n):
    """every base element once as element B - 1 or as its partner, over the maps (of any sizes)"""
    seen = set()
    for m in maps:
        seen |= coverage([m], n)[1]
    assert seen == set(range(n)), f"base elements never in the last sweep pair: {sorted(set(range(n)) - seen)}"


def draw(n, B, seed, groups=None):
    """A seeded index map [B] into n base elements for a batch large enough to hold, alone, every
    base element at every residue of b mod 4 and every ordered pair of sweep partners (both
    asserted).  Element B - 1 is base element seed mod n: a case's batch sizes, drawn with
    consecutive seeds, bring every base element there (assert_last).  n: odd and coprime to 64, so
    that no power-of-two stride of the batch lands on one base element only."""
    assert n % 2 == 1 and n >= 3 and np.gcd(n, 64) == 1, f"n = {n}: odd and coprime to 64 (5 or 7)"
    need = pairs_needed(n, groups)
    assert B >= need, f"B = {B} cannot hold every ordered pair of {n} base elements ({need} slots): use draws()"
    rng = np.random.default_rng([seed, n, B])
    index = rng.integers(0, n, B)
    at = 0
    for g in _groups(n, groups):  # a layout's pairs one after the other: its elements stay paired as written
        for i in g:
            for j in g:
                index[at], index[at + 1] = i, j
                at += 2
    index[B - 1] = seed % n
    index = index.astype(np.int64)
    # residues the pairs and the seeded rest have left out (several layouts, small B): placed behind the pairs
    free = at
    for i in range(n):
        for r in range(4):
            if not np.any(index[r::4] == i):
                free += (r - free) % 4
                assert free < B - 1
                index[free] = i
                free += 1
    assert_residues([index], n)
    assert_pairs([index], n, groups)
    return index


def draws(n, B, seed, groups=None):
    """The index maps to run at batch size B: draw's one map where B holds the full coverage, else
    (B < pairs_needed) the n rotations index[b] = (b + seed + r) mod n, which together put every base
    element at every b — every residue mod 4 the batch has, B - 1 included (asserted) — and form the
    sweep pairs that fit."""
    if B >= pairs_needed(n, groups):
        return [draw(n, B, seed, groups)]
    assert n % 2 == 1 and n >= 3 and np.gcd(n, 64) == 1, f"n = {n}: odd and coprime to 64 (5 or 7)"
    maps = [((np.arange(B) + seed + r) % n).astype(np.int64) for r in range(n)]
    assert_residues(maps, n)
    assert_last(maps, n)
    return maps


# ---- tiled problems ------------------------------------------------------------------------------------
PER_ELEMENT = ("contacts", "x0", "Xbar", "Ubar")
REFS = ("ref_x", "ref_u", "ref_foot")


def tile(prob, index):
    """The batch whose element b is element index[b] of `prob` (hsddp.synthetic.make_batch, uniform or
    mixed=True, or make_layout_batch).  A shared reference stays shared; per-element references and
    layouts are tiled with their elements."""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    n = int(prob["batch"])
    assert index.size > 0 and index.min() >= 0 and index.max() < n, "index outside the base batch"
    if "ref_table" in prob:
        raise ValueError("tile: batches with a reference table are not handled")
    out = dict(prob)
    out["batch"] = int(index.size)
    for k in PER_ELEMENT:
        out[k] = np.ascontiguousarray(prob[k][index])
    for k in REFS:
        out[k] = prob[k] if prob[k].shape[0] == 1 else np.ascontiguousarray(prob[k][index])
    if prob.get("K") is not None:
        out["K"] = np.ascontiguousarray(prob["K"][index])
    if len(prob.get("gaits", ())) == n:
        out["gaits"] = [prob["gaits"][i] for i in index]
    if prob.get("layouts") is not None:
        lays = [list(prob["layouts"][i]) for i in index]
        # the arrays keep the base batch's strides: the tile must hold an element of the largest layout
        assert max(len(h) for h in lays) == len(max(prob["layouts"], key=len)), "no element of the largest layout in the tile"
        out["layouts"] = lays
        out["horizons"] = lays[0]
    return out


def layout_groups_of(prob):
    """the base elements of each layout ([[...], ...]), or None for a batch with one layout"""
    if prob.get("layouts") is None:
        return None
    out = {}
    for b, h in enumerate(prob["layouts"]):
        out.setdefault(tuple(h), []).append(b)
    return list(out.values())


# ---- records -------------------------------------------------------------------------------------------
def record_fields(Kc, S_cap, fp32, record_bytes):
    """{name: (byte offset, dtype, shape)} of a record's payload (hsddp_elements.h: record_layout; every
    piece 16-byte aligned, the header and the record whole 128-byte lines)."""
    real = np.float32 if fp32 else np.float64
    pieces = [("K", real, (Kc, KCW))]
    pieces += [(k, np.float64, (S_cap, NX)) for k in ("Xn", "Xw", "Dw", "dX", "rx", "ru")]
    pieces += [("rf", np.float64, (S_cap, 12)), ("d32", np.float32, (S_cap if fp32 else 0, NX))]
    pieces += [(k, np.float64, (S_cap,)) for k in ("scost", "sfeas", "sviol")] + [("sdiv", np.int32, (S_cap,))]
    pieces += [(k, np.float64, (Kc, NX)) for k in ("Un", "Uw", "dU", "du")]
    pieces += [("rdel", np.float64, (Kc, 20)), ("reps", np.float64, (Kc, 20)), ("cfu", np.float64, (Kc, 12)),
               ("cff", np.int32, (Kc,))]
    pieces += [("tdm", np.int32, (MAXP, MTD)), ("als", np.float64, (MAXP, MTD, 4)), ("all", np.float64, (MAXP, MTD, 4)),
               ("th", np.float64, (MAXP, 4)), ("con", np.int32, (MAXP + 1, 4)), ("x0", np.float64, (NX,)),
               ("el", ELEM_STATE, ()), ("sel", np.int32, ()), ("hist", np.float32, (REC_HIST, 4))]
    out, at = {}, 0
    for name, dt, shape in pieces:
        out[name] = (at, np.dtype(dt), shape)
        at += (int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize + 15) & ~15
    header = (record_bytes - at) // 128 * 128  # the header's lines: the only multiple of 128 that fits
    assert header >= 128 and (header + at + 127) & ~127 == record_bytes, \
        f"record layout: payload {at} bytes does not fit the library's {record_bytes}-byte record"
    return {k: (header + o, dt, shape) for k, (o, dt, shape) in out.items()}


def parse_records(rec, Kc, S_cap, fp32):
    """records [m][bytes] (uint8) -> {name: array [m][...]} (views)"""
    rec = np.ascontiguousarray(rec)
    m, nbytes = rec.shape
    out = {}
    for name, (o, dt, shape) in record_fields(Kc, S_cap, fp32, nbytes).items():
        cnt = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        out[name] = rec[:, o:o + cnt].view(dt).reshape((m,) + shape) if cnt else np.zeros((m,) + shape, dt)
    return out


SLOT_FIELDS = ("Xn", "Xw", "Dw", "dX", "rx", "ru", "rf", "d32", "scost", "sfeas", "sviol", "sdiv")  # [S_cap]: own S
KNOT_FIELDS = ("K", "Un", "Uw", "dU", "du", "rdel", "reps")                                        # [Kc]
OVR_FIELDS = ("cfu", "cff")                                                                      # [Kc], read while ovr
PHASE_FIELDS = ("tdm", "als", "all", "th")                                                       # [MAXP]: own P
WHOLE_FIELDS = ("x0", "el", "sel", "hist")
NO_GAINS = tuple(f for f in SLOT_FIELDS + KNOT_FIELDS + OVR_FIELDS + PHASE_FIELDS + ("con",) + WHOLE_FIELDS if f != "K")


def _bytes(a):
    """[m][...] -> [m][rows][bytes per row] (rows = the second axis, 1 for per-element fields)"""
    m = a.shape[0]
    rows = a.shape[1] if a.ndim > 1 else 1
    return np.ascontiguousarray(a).view(np.uint8).reshape(m, rows, -1) if a.size else np.zeros((m, rows, 0), np.uint8)


def _layouts(s, elements=None):
    n, hz, ss, re = s._layout_arrays()
    if elements is not None:
        n, hz, ss, re = n[elements], hz[elements], ss[elements], re[elements]
    return {"n_phases": n, "horizons": hz, "shooting": ss, "reach_end": re}


def snapshot(s, check=True, fp32=False):
    """Every element's record of a (small) handle, parsed, with the host's layout arrays.  check: the
    parse is right — the fields equal what the download calls return for the same handle.  fp32: the
    handle was made with riccati_fp32."""
    rec = s.export_elements(np.arange(s.B))
    S_cap = s.Kc + MAXP
    snap = parse_records(rec, s.Kc, S_cap, fp32)
    snap["_lay"] = _layouts(s)
    snap["_Kc"], snap["_S_cap"], snap["_fp32"] = s.Kc, S_cap, fp32
    if check:
        S, P = s.S, s.P
        tr, wk, ei, cp, rf = s.trajectory(), s.working(), s.element_info(), s.constraint_params(), s.references()
        pairs = [("Xn", tr["Xbar"], S), ("Un", tr["Ubar"], None), ("Xw", wk["X"], S), ("Uw", wk["U"], None),
                 ("Dw", wk["Defect"], S), ("dX", wk["dX"], S), ("dU", wk["dU"], None), ("rdel", cp["reb_delta"], None),
                 ("reps", cp["reb_eps"], None), ("tdm", cp["td_mask"], P), ("als", cp["al_sigma"], P),
                 ("all", cp["al_lambda"], P)]
        for f, g in (("rx", "ref_x"), ("ru", "ref_u"), ("rf", "ref_foot")):  # (a shared reference: in every record)
            pairs.append((f, np.broadcast_to(rf[g], (s.B,) + rf[g].shape[1:]), S))
        for f, want, rows in pairs:
            got = snap[f] if rows is None else snap[f][:, :rows]
            assert np.array_equal(got, want, equal_nan=True), f"record field {f} is not what the download returns"
        for f, g in (("cost", "cost"), ("feas", "feas"), ("merit", "merit"), ("max_t", "max_tconstr"), ("max_p", "max_pconstr"),
                     ("iters", "iters"), ("outer_iters", "outer_iters"), ("status", "status"), ("n_ls", "n_ls_trials")):
            assert np.array_equal(snap["el"][f], ei[g], equal_nan=True), f"ElemState::{f} is not element_info's {g}"
        # the compact gains: the 288 entries of a knot that may be non-zero in the expanded 24 x 24 block
        big = np.sort(np.abs(tr["K"]).reshape(s.B, s.Kc, -1), axis=-1)[..., -KCW:]
        assert np.array_equal(big, np.sort(np.abs(snap["K"].astype(np.float64)), axis=-1)), "record field K"
        assert np.all(np.sort(np.abs(tr["K"]).reshape(s.B, s.Kc, -1), axis=-1)[..., :-KCW] == 0)
        assert np.array_equal(snap["con"][:, :P + 1], s.phase_info()["contacts"])
        assert np.array_equal(snap["x0"], s.prob["x0"])
    return snap


def differences(rec, base, index, fields=None):
    """{field: [positions in the chunk]} where parsed records `rec` differ from the base elements
    `index` of snapshot `base`, byte for byte, over each element's own rows."""
    idx = np.asarray(index)
    lay = base["_lay"]
    P_own = lay["n_phases"][idx]
    S_own = lay["horizons"][idx].sum(1) + P_own  # sum(N_i + 1) over the element's phases
    ovr = base["el"]["ovr"][idx] != 0
    bad = {}
    for f in (fields or SLOT_FIELDS + KNOT_FIELDS + OVR_FIELDS + PHASE_FIELDS + ("con",) + WHOLE_FIELDS):
        a, b = _bytes(rec[f]), _bytes(base[f][idx])
        ne = (a != b).any(-1)  # [m][rows]
        rows = np.arange(ne.shape[1])[None, :]
        if f in SLOT_FIELDS:
            ne &= rows < S_own[:, None]
        elif f in PHASE_FIELDS:
            ne &= rows < P_own[:, None]
        elif f == "con":
            ne &= rows <= P_own[:, None]
        elif f in OVR_FIELDS:
            ne &= ovr[:, None]
        if ne.any():
            bad[f] = np.flatnonzero(ne.any(1)).tolist()
            if f == "el":  # ... and which of ElemState's fields
                for k in ELEM_STATE.names:
                    pos = np.flatnonzero((_bytes(rec[f][k]) != _bytes(base[f][k][idx])).any((1, 2)))
                    if pos.size:
                        bad["el." + k] = pos.tolist()
    return bad


def same(big, base, index, elements=None, chunk=256, fields=None):
    """Elements `elements` (default: all) of the tiled handle `big` equal base elements index[b] of
    snapshot(base handle), bit for bit: their records in chunks of `chunk` (host memory stays
    bounded), and their layouts as the host holds them.  fields: a subset of the record fields
    (NO_GAINS: all but the gain rows)."""
    index = np.asarray(index)
    el = np.arange(big.B) if elements is None else np.asarray(elements, dtype=np.int64)
    assert big.Kc == base["_Kc"]
    lay, blay = _layouts(big, el), base["_lay"]
    for k in lay:
        ne = np.flatnonzero((lay[k] != blay[k][index[el]]).reshape(len(el), -1).any(1))
        assert ne.size == 0, (k, el[ne][:8].tolist())
    for at in range(0, len(el), chunk):
        part = el[at:at + chunk]
        rec = parse_records(big.export_elements(part), big.Kc, base["_S_cap"], base["_fp32"])
        bad = differences(rec, base, index[part], fields)
        assert not bad, {f: [(int(part[j]), int(index[part[j]])) for j in pos[:8]] for f, pos in bad.items()}
