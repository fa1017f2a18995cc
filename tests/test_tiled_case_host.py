"""CPU checks of tests/tiled_case.py (the helper behind tests/test_gpu_batch_sizes.py): the coverage
`draw` / `draws` assert really is asserted, `tile` of the three batch kinds puts base element
index[b] at b, the record layout `same` parses is the library's (hsddp_elements.h, through the C++
compiler), and the oracle — which knows nothing of batches — gives equal copies equal results on a
tiled problem, so the base problems are built identically wherever they land."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import tiled_case as TC
from hsddp import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TROT = ("trot", 4, 16)
JUMP = ("jump", 8, 8)


def _bases():
    """the three batch kinds, five elements each: one layout and a shared reference, one layout and
    per-element references, per-element layouts"""
    return {"uniform": syn.make_batch(5, 4, 16, "trot"),
            "mixed": syn.make_batch(5, 4, 16, "trot", mixed=True),
            "layouts": syn.make_layout_batch([TROT, JUMP, TROT, JUMP, JUMP])}


# ---- draw / draws --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(5, 52), (5, 53), (5, 511), (5, 2049), (7, 100), (7, 4097)])
def test_draw_covers_what_it_promises(n, B):
    maps = [TC.draw(n, B, seed) for seed in range(n)]
    for seed, m in enumerate(maps):
        assert m.shape == (B,) and m.min() == 0 and m.max() == n - 1
        assert m[B - 1] == seed % n
        res, last, pairs = TC.coverage([m], n)
        assert all(r == {0, 1, 2, 3} for r in res)
        assert pairs == {(i, j) for i in range(n) for j in range(n)}
        assert np.array_equal(m, TC.draw(n, B, seed))  # seeded
    TC.assert_last(maps, n)
    assert any(not np.array_equal(maps[0][:B - 1], m[:B - 1]) for m in maps[1:])


def test_draw_with_layout_groups_pairs_within_a_layout():
    groups = [[0, 2], [1, 3, 4]]
    m = TC.draw(5, 513, 3, groups)
    pairs = TC.sweep_pairs(m, groups)
    assert len(pairs) == TC.n_pairs(m, groups)
    for a, c in pairs:  # partners share a layout; at most one lone element per layout
        assert c < 0 or any(m[a] in g and m[c] in g for g in groups)
    assert sum(c < 0 for _, c in pairs) <= 2
    _, _, got = TC.coverage([m], 5, groups)
    assert got == {(i, j) for g in groups for i in g for j in g}
    nt = int(np.isin(m, groups[0]).sum())
    assert len(pairs) == (nt + 1) // 2 + (513 - nt + 1) // 2


def test_draw_refuses_what_would_test_less():
    with pytest.raises(AssertionError, match="coprime"):
        TC.draw(4, 1000, 0)
    with pytest.raises(AssertionError, match="coprime"):
        TC.draw(6, 1000, 0)
    with pytest.raises(AssertionError, match="cannot hold"):
        TC.draw(5, 51, 0)
    with pytest.raises(AssertionError, match="cannot hold"):
        TC.draw(7, 64, 0)
    with pytest.raises(AssertionError, match="partition"):
        TC.draw(5, 1000, 0, [[0, 1], [3, 4]])


def test_the_coverage_assertions_fail_on_bad_maps():
    B = 400
    with pytest.raises(AssertionError, match="residues"):  # base element b mod 4 at b: one residue each
        TC.assert_residues([np.arange(B) % 4], 5)
    stripes = np.arange(B) % 5  # every residue, but element i is only ever followed by i + 1
    TC.assert_residues([stripes], 5)
    with pytest.raises(AssertionError, match="never formed"):
        TC.assert_pairs([stripes], 5)
    with pytest.raises(AssertionError, match="last sweep pair"):
        TC.assert_last([stripes, stripes], 5)
    even = TC.draw(5, 400, 2)
    assert TC.coverage([even], 5)[1] == {int(even[398]), 2}  # B even: B - 1 and its partner B - 2
    odd = TC.draw(5, 401, 2)
    assert TC.coverage([odd], 5)[1] == {2}                   # B odd: B - 1 alone in its pair


@pytest.mark.parametrize("B", [3, 4, 16, 17])
def test_draws_for_small_batches_covers_by_rotation(B):
    maps = TC.draws(5, B, 7)
    assert len(maps) == 5 and all(m.shape == (B,) for m in maps)
    for b in range(B):  # every base element at every position
        assert {int(m[b]) for m in maps} == set(range(5))
    assert len(TC.draws(5, 52, 7)) == 1


# ---- tile ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "mixed", "layouts"])
def test_tile_round_trips(kind):
    prob = _bases()[kind]
    groups = TC.layout_groups_of(prob)
    index = TC.draw(5, 61, 1, groups)
    big = TC.tile(prob, index)
    assert big["batch"] == 61 and prob["batch"] == 5  # (the base is untouched)
    for k in ("dt", "S", "Kc"):
        assert big[k] == prob[k]
    shared = prob["ref_x"].shape[0] == 1
    assert shared == (kind == "uniform")
    for k in TC.REFS:
        if shared:
            assert big[k] is prob[k]  # the reference stays shared
        else:
            assert big[k].shape[0] == 61
    if kind != "layouts":
        for b in range(61):
            for k in TC.PER_ELEMENT + (() if shared else TC.REFS):
                assert np.array_equal(big[k][b], prob[k][index[b]]), (k, b)
        assert big["gaits"] == [prob["gaits"][i] for i in index]
        # and back: indexing the tile by one position of every base element gives the base
        first = [int(np.flatnonzero(index == i)[0]) for i in range(5)]
        back = TC.tile(big, first)
        for k in TC.PER_ELEMENT + (() if shared else TC.REFS):
            assert np.array_equal(back[k], prob[k]), k
        return
    # per-element layouts: each layout's elements as an ordinary batch (sub_batch) equal the base's
    assert big["layouts"] == [prob["layouts"][i] for i in index] and big["horizons"] == big["layouts"][0]
    gb, gp = syn.layout_groups(big), syn.layout_groups(prob)
    assert set(gb) == set(gp) and len(gp) == 2
    for hz, el in gb.items():
        assert all(index[b] in gp[hz] for b in el)
        a, w = syn.sub_batch(big, el, hz), syn.sub_batch(prob, [index[b] for b in el], hz)
        for k in ("contacts", "x0", "ref_x", "ref_u", "ref_foot", "Xbar", "Ubar"):
            assert np.array_equal(a[k], w[k]), (hz, k)
    with pytest.raises(AssertionError, match="largest layout"):
        TC.tile(prob, [0, 2, 0])
    with pytest.raises(AssertionError, match="outside"):
        TC.tile(prob, [0, 5])


# ---- the oracle on a tiled problem ---------------------------------------------------------------------
FIELDS = ("Xbar", "Ubar", "K", "X", "U", "dX", "dU", "Defect", "reb_delta", "reb_eps", "al_sigma", "al_lambda", "td_mask",
          "grf_g", "td_h", "cost", "feas", "merit", "max_tconstr", "max_pconstr", "iters", "outer_iters", "status",
          "n_ls_trials")


@pytest.mark.parametrize("kind", ["uniform", "mixed", "layouts"])
def test_oracle_gives_equal_copies_equal_results(kind):
    prob = _bases()[kind]
    n = 5
    index = np.concatenate([np.random.default_rng(k).permutation(n) for k in range(3)])  # 3 x n elements
    big = TC.tile(prob, index)
    opt = O.default_options(no_early_exit=1, max_AL_iter=1, max_DDP_iter=3)

    def solve(p):
        if p.get("layouts") is None:
            return {b: {f: r[f][b] for f in FIELDS} for r in [O.solve_batch(p, opt, n_threads=8)] for b in range(p["batch"])}
        out = {}
        for hz, el in syn.layout_groups(p).items():
            r = O.solve_batch(syn.sub_batch(p, el, hz), opt, n_threads=8)
            out.update({b: {f: r[f][j] for f in FIELDS} for j, b in enumerate(el)})
        return out

    base, tiled = solve(prob), solve(big)
    assert len(tiled) == 3 * n
    for b in range(3 * n):
        for f in FIELDS:
            assert np.array_equal(tiled[b][f], base[index[b]][f], equal_nan=True), (b, f)
    costs = [float(base[i]["cost"]) for i in range(n)]
    assert len(set(costs)) == n  # five different problems, not one five times


# ---- the record layout ---------------------------------------------------------------------------------
NAMES = ["K", "Xn", "Xw", "Dw", "dX", "rx", "ru", "rf", "d32", "scost", "sfeas", "sviol", "sdiv", "Un", "Uw", "dU", "du",
         "rdel", "reps", "cfu", "cff", "tdm", "als", "all", "th", "con", "x0", "el", "sel", "hist"]


def _c_layout(tmp_path, Kc, fp32):
    """record_layout(Kc, Kc + MAXP, fp32) of hsddp_elements.h through the C++ compiler: [bytes, the
    offsets of NAMES, sizeof(ElemState), MAXP, MTD, KCW, REC_HIST, NX]"""
    names = NAMES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include "hsddp_elements.h"\nint main(){\n'
                   f'const hsddp::RecordLayout R = hsddp::record_layout({Kc}, {Kc} + hsddp::MAXP, {fp32});\n'
                   'std::printf("%zu\\n", R.bytes);\n' + "".join(f'std::printf("%zu\\n", R.{f});\n' for f in names) +
                   'std::printf("%zu %d %d %d %d %d\\n", sizeof(hsddp::ElemState), hsddp::MAXP, hsddp::MTD, hsddp::KCW, '
                   'hsddp::REC_HIST, hsddp::NX);\nreturn 0;}\n')
    exe = tmp_path / "layout"
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "hkd-mpc_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    return [int(v) for v in out]


@pytest.mark.parametrize("Kc,fp32", [(64, 0), (200, 0), (20, 1)])
def test_record_fields_are_hsddp_elements_h(tmp_path, Kc, fp32):
    """record_layout of hsddp_elements.h against tiled_case.record_fields"""
    vals, names = _c_layout(tmp_path, Kc, fp32), NAMES
    assert vals[-6:] == [TC.ELEM_STATE.itemsize, TC.MAXP, TC.MTD, TC.KCW, TC.REC_HIST, TC.NX]
    fields = TC.record_fields(Kc, Kc + TC.MAXP, bool(fp32), vals[0])
    assert [fields[f][0] for f in names] == vals[1:1 + len(names)]
    with pytest.raises(AssertionError, match="record layout"):
        TC.record_fields(Kc + 1, Kc + TC.MAXP, bool(fp32), vals[0])  # (another handle's record size)


def test_differences_sees_own_rows_and_only_those(tmp_path):
    """records of random bytes: a copy equals its base; one flipped bit in an element's own rows is
    found under its field's name; the same in padding rows, the header, or the stored GRF forces of an
    element with ovr = 0 is not"""
    Kc = 64
    nbytes = _c_layout(tmp_path, Kc, 0)[0]
    fields = TC.record_fields(Kc, Kc + TC.MAXP, False, nbytes)
    rng = np.random.default_rng(0)
    base_rec = rng.integers(0, 256, (2, nbytes), dtype=np.uint8)
    base = TC.parse_records(base_rec, Kc, Kc + TC.MAXP, False)
    assert base["K"].shape == (2, Kc, TC.KCW) and base["Xn"].shape == (2, Kc + TC.MAXP, 24) and base["el"].shape == (2,)
    base["el"]["ovr"][:] = [0, 1]
    hz = np.zeros((2, 16), np.int32)
    hz[0, :4], hz[1, :8] = 16, 8  # trot 4 x 16: S = 68, P = 4; jump 8 x 8: S = 72, P = 8
    base["_lay"] = {"n_phases": np.array([4, 8], np.int32), "horizons": hz}
    index = np.array([1, 0, 0, 1, 1])

    def tiled():
        return np.ascontiguousarray(base_rec[index])

    def diff(rec):
        return TC.differences(TC.parse_records(rec, Kc, Kc + TC.MAXP, False), base, index)

    assert diff(tiled()) == {}

    def flip(f, pos, row, found):
        o, dt, shape = fields[f]
        per_row = int(np.prod(shape[1:], dtype=np.int64)) * dt.itemsize if shape else dt.itemsize
        rec = tiled()
        rec[pos, o + row * per_row + per_row - 1] ^= 0x10
        assert diff(rec) == ({f: [pos]} if found else {}), (f, pos, row)

    for f in ("Xn", "Xw", "Dw", "dX", "rx", "ru", "rf", "scost", "sfeas", "sviol", "sdiv"):
        flip(f, 1, 67, True)    # a trot copy's last slot
        flip(f, 1, 68, False)   # ... and its first padding row
        flip(f, 0, 71, True)    # a jump copy's last slot
        flip(f, 0, 72, False)
    for f in ("K", "Un", "Uw", "dU", "du", "rdel", "reps"):
        flip(f, 2, 0, True)
        flip(f, 4, Kc - 1, True)
    for f in ("tdm", "als", "all", "th"):
        flip(f, 2, 3, True)
        flip(f, 2, 4, False)
        flip(f, 3, 7, True)
        flip(f, 3, 8, False)
    flip("con", 2, 4, True)     # rows 0 .. P: the next contact after the last phase
    flip("con", 2, 5, False)
    for f in ("cfu", "cff"):
        flip(f, 0, 5, True)     # a copy of base element 1 (ovr = 1)
        flip(f, 1, 5, False)    # ... of base element 0 (ovr = 0): arbitrary contents
    for f in ("x0", "sel", "hist"):
        flip(f, 3, 0, True)
    rec = tiled()
    rec[3, fields["el"][0] + TC.ELEM_STATE.fields["reg"][1]] ^= 1  # ElemState: the field is named too
    assert diff(rec) == {"el": [3], "el.reg": [3]}
    rec = tiled()
    rec[:, :fields["K"][0]] ^= 0xFF  # the header
    assert diff(rec) == {}
