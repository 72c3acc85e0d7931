"""The three world-map stages - occupancy_fuse, occupancy_match, clearance_paths - where their batch and capacity loops turn over: the
fuse's cull round of 64 frames, the match's compaction workgroups of 4096 cells, its lists at capacity, its partial maxima past 2048 and
its int32 chunk sums at the ends of int16, and the path check's (step, disc) walk at disc counts that do not divide 64 and at the longest
path.  The cases come from tests/map_stage_cases.py; the CPU tests assert that each is what it claims to be.

The reference is always the numpy definition in stereo_vision.sv on the CPU, and every comparison is bit for bit: everything here is
integers behind double arithmetic in a stated order (test_occupancy_map.py, test_map_match.py and test_clearance.py say why)."""
import numpy as np
import pytest

import map_stage_cases as mc
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_occupancy_map import SMALL
from test_occupancy_map import _counted as _fuse_counted, _gpu as _fuse_gpu, _same as _fuse_same
from test_map_match import KEYS as MATCH_KEYS, SMALL_MAPS, _bits, _small_words
from test_map_match import _counted as _match_counted, _gpu as _match_gpu, _same as _match_same
from test_clearance import PATH_COUNTS, PATH_KEYS, _paths_gpu, _poses_around

F = 65535
FULL = np.uint64(2 ** 64 - 1)


# ---------------------------------------------------------------------------------------------------------------- fuse

def _fuse_case(sv, case, B, name, touching):
    """(state, poses, L0, S0): the hand-placed patterns on a map with a past, the runs under the clamp ("all", "mix") on a fresh one."""
    frame, words = SMALL[case]
    _, _, _, frows, fcols = sv.occupancy_frame_grid(frame)
    state, poses = mc.fuse_batch(case, B, touching, frows, fcols)
    if name in ("all", "mix"):
        return state, poses, None, None
    rng = np.random.default_rng(B)
    return state, poses, rng.integers(-200, 351, (37, 29)).astype(np.int16), rng.integers(-1, 9, (37, 29)).astype(np.int32)


@pytest.mark.parametrize("case", sorted(SMALL))
def test_the_fuse_batches_are_what_the_issue_asks_for(sv, case):
    """Per B: the ballots of the hand-placed patterns have the stated shapes, the runs reach both ends of the clamp and hold them, and the
    order of the frames shows."""
    frame, words = SMALL[case]
    for B in mc.FUSE_BATCHES:
        patterns = mc.fuse_patterns(B)
        assert len(patterns["mix"]) >= 24 and {"bit0", "all", "none", "last", "mix"} <= set(patterns) and (B < 65 or {"bit63", "second_round", "b63_b64"} <= set(patterns)) and (B > 63 or "bit63" not in patterns)
        for name, touching in patterns.items():
            state, poses, L0, S0 = _fuse_case(sv, case, B, name, touching)
            ballots = mc.cull_ballots(sv, poses, frame, words)
            assert ballots.shape == (19 * 1, (B + 63) // 64)
            union = np.bitwise_or.reduce(ballots, 0)
            want = np.zeros_like(union)
            for b in touching:
                want[b // 64] |= np.uint64(1) << np.uint64(b % 64)
            assert np.array_equal(union, want), (B, name)  # the frames that touch, and no other, pass some strip's cull
            if name == "all":  # a full ballot, bit 63 included, in every whole round of one strip; the last round is the masked tail
                assert (ballots[:, :B // 64] == FULL).all(1).any() and (B % 64 == 0 or (ballots[:, -1] == np.uint64(2 ** (B % 64) - 1)).any())
            elif name != "mix":  # one strip sees exactly the stated bits; no strip sees others
                assert (ballots == want[None]).all(1).any() and ((ballots & ~want[None]) == 0).all()
            want_map = sv.occupancy_fuse(state, poses, frame, words, L0, S0, seq0=mc.INT_MAX - B)
            assert (want_map["last_seen"] == mc.INT_MAX - B + touching[-1]).any() if touching else L0 is not None and _bits(want_map["logodds"], L0)
            assert mc.seen_pairs(sv, poses, frame, words) > 0 or not touching
            if name in ("all", "mix"):
                backwards = sv.occupancy_fuse(state[::-1], poses[::-1], frame, words, seq0=mc.INT_MAX - B)
                assert not np.array_equal(want_map["logodds"], backwards["logodds"]), (B, name)
                assert (want_map["logodds"] == words["l_max"]).any() and (want_map["logodds"] == words["l_min"]).any(), (B, name)


def test_the_fuse_geometries_are_what_the_issue_asks_for(sv):
    geo = mc.fuse_geometries(sv)
    assert set(geo) == {"tiny_frame", "map_cell_x64", "frame_cell_x64", "on_the_border", "no_rotation", "far_pp", "far_mm", "far_pm"}
    for name, (frame, words, poses) in geo.items():
        seen = np.array([mc.seen_pairs(sv, poses[k:k + 1], frame, words) for k in range(len(poses))])
        assert (seen > 0).sum() >= 3 and (seen == 0).any() and seen[0] > 0 and seen[1] > 0, (name, seen.tolist())
        many = mc.geometry_batch(poses)
        assert many.shape == (65, 4) and many[63].tolist() == poses[0].tolist() and many[64].tolist() == poses[1].tolist()
    frame, words, _ = geo["tiny_frame"]
    assert sv.occupancy_frame_grid(frame)[3:] == (2, 2)
    for bad in (dict(x_range=(0, 0)), dict(scale=0)):  # nothing smaller is admitted
        with pytest.raises(ValueError):
            sv.occupancy_frame_grid(dict(frame, **bad))
    assert geo["map_cell_x64"][0]["scale"] == 64 * geo["map_cell_x64"][1]["scale"] and geo["frame_cell_x64"][1]["scale"] == 64 * geo["frame_cell_x64"][0]["scale"]
    # on the border: under the exact quarter turns whole lines of centres have a coordinate equal to a bound of the frame, and are not seen
    frame, words, poses = geo["on_the_border"]
    (fx0, fx1), (fy0, fy1), _, _, _ = sv.occupancy_frame_grid(frame)
    Xw, Yw = sv.occupancy_map_centres(words)
    quarter = [k for k in range(len(poses) - 1) if set(np.abs(poses[k, 2:]).tolist()) == {0.0, 1.0}]  # the last pose is far away
    assert len(quarter) == 8
    Xf, Yf = mc._frame_axes(sv, poses[quarter], frame, words, Xw, Yw)
    inside_y, inside_x = (Yf > fy0) & (Yf < fy1), (Xf > fx0) & (Xf < fx1)
    on = np.stack([((Xf == fx0) & inside_y).any(axis=(1, 2)), ((Xf == fx1) & inside_y).any(axis=(1, 2)), ((Yf == fy0) & inside_x).any(axis=(1, 2)), ((Yf == fy1) & inside_x).any(axis=(1, 2))])
    assert (on.sum(0) >= 2).all() and (on.sum(1) >= 3).all(), on.astype(int).tolist()  # each pose puts centres on two of the four borders or more, each border has three poses or more
    yaws = np.arctan2(poses[:8, 3], poses[:8, 2]) / (np.pi / 4)
    assert np.allclose(yaws, np.rint(yaws)) and len(set(np.rint(yaws).astype(int) % 8)) == 8
    n = (geo["no_rotation"][2][:, 2:] ** 2).sum(1)
    assert (n > 1).any() and (n < 1).any() and not (n == 1).any()
    assert {(geo[k][1]["top"], geo[k][1]["left"]) for k in ("far_pp", "far_mm", "far_pm")} == {(2 ** 24 - 1, 2 ** 24 - 1), (1 - 2 ** 24, 1 - 2 ** 24), (2 ** 24 - 1, 1 - 2 ** 24)}
    with pytest.raises(ValueError):
        sv.occupancy_map_words(dict(geo["far_pp"][1], top=2 ** 24))
    # the map shapes: a shift of rows or more leaves nothing of the map coming in
    rng = np.random.default_rng(3)
    for rows, cols in [(r, c) for r in mc.MAP_ROWS for c in mc.MAP_COLS] + list(mc.LONG_MAPS):
        shifts = mc.map_shifts(rows, cols)
        gone = [s for s in shifts if mc.nothing_survives(s, rows, cols)]
        assert len(gone) >= 7 and (rows - 1, 0) in shifts and (1 - rows, 0) in shifts and (0, cols - 1) in shifts and (rows, 0) in gone and (-rows, 0) in gone
        L0, S0 = rng.integers(1, 351, (rows, cols)).astype(np.int16), rng.integers(0, 9, (rows, cols)).astype(np.int32)
        for s in shifts:
            kept = sv.occupancy_scroll(S0, s, -1)
            assert (kept >= 0).any() != mc.nothing_survives(s, rows, cols), (rows, cols, s)


def _both_culls(sv, eng, state, poses, frame, words, L0=None, S0=None, seq0=0, shift=(0, 0), what=None):
    """The kernel with the cull on and off against the definition, last_seen included, and the lookups each made against the bounds."""
    want = sv.occupancy_fuse(state, poses, frame, words, L0, S0, seq0=seq0, shift=shift)
    on, n_on = _fuse_counted(eng, True, lambda: _fuse_gpu(eng, state, poses, frame, words, L0, S0, seq0, shift))
    off, n_off = _fuse_counted(eng, False, lambda: _fuse_gpu(eng, state, poses, frame, words, L0, S0, seq0, shift))
    assert _fuse_same(on, want) and _fuse_same(off, want), (what, _fuse_same(on, want), _fuse_same(off, want))
    n_seen = mc.seen_pairs(sv, poses, frame, words)
    assert n_off == words["rows"] * words["cols"] * len(poses) and n_seen <= n_on <= n_off, (what, n_seen, n_on, n_off)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("B", mc.FUSE_BATCHES)
@pytest.mark.parametrize("case", sorted(SMALL))
def test_fuse_batches_around_the_cull_round(sv, eng, case, B):
    """Every pattern of touching frames, with the cull on and off, at seq0 = INT_MAX - B - the largest the entry admits."""
    frame, words = SMALL[case]
    for name, touching in mc.fuse_patterns(B).items():
        state, poses, L0, S0 = _fuse_case(sv, case, B, name, touching)
        _both_culls(sv, eng, state, poses, frame, words, L0, S0, seq0=mc.INT_MAX - B, what=(case, B, name))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SMALL))
def test_fuse_split_at_the_cull_round(sv, eng, case):
    """One call with B = 130 equals calls of 64 + 64 + 2 and of 65 + 65 on slices of the same tensors, enqueued back to back with seq0
    advanced.  In the calls of 65 the lanes behind the batch's last frame stand in front of poses and states of frames that are there
    and touch the map: only the b < B of the cull keeps them out."""
    import torch
    frame, words = SMALL[case]
    B = 130
    touching = list(range(B))
    state, poses = mc.fuse_batch(case, B, touching, *sv.occupancy_frame_grid(frame)[3:])
    seq0 = mc.INT_MAX - B
    want = sv.occupancy_fuse(state, poses, frame, words, seq0=seq0)
    assert (want["logodds"] == 350).any() and (want["logodds"] == -200).any()
    twice = sv.occupancy_fuse(state[65:128], poses[65:128], frame, words, want["logodds"], want["last_seen"], seq0=seq0)
    assert not np.array_equal(twice["logodds"], want["logodds"])  # frames 65 .. 127 applied once more would show
    t_state, t_poses = _cuda(state), _cuda(poses)
    for steps in ((130,), (64, 64, 2), (65, 65)):
        res, b = None, 0
        for n in steps:
            res = eng.occupancy_fuse(t_state[b:b + n], t_poses[b:b + n], frame, words, None if res is None else res.logodds, None if res is None else res.last_seen, seq0=seq0 + b)
            b += n
        torch.cuda.synchronize()
        assert _fuse_same({"logodds": res.logodds.cpu().numpy(), "last_seen": res.last_seen.cpu().numpy()}, want), steps


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_frame", "map_cell_x64", "frame_cell_x64", "on_the_border", "no_rotation", "far_pp", "far_mm", "far_pm"])
def test_fuse_geometry_at_the_culls_margin(sv, eng, name):
    """Each pose alone (B = 1) and all of them again and again over B = 65, with the cull on and off."""
    frame, words, poses = mc.fuse_geometries(sv)[name]
    _, _, _, frows, fcols = sv.occupancy_frame_grid(frame)
    rng = np.random.default_rng(len(name))
    L0, S0 = rng.integers(-200, 351, (37, 29)).astype(np.int16), rng.integers(-1, 9, (37, 29)).astype(np.int32)
    touched = 0
    for k, pose in enumerate(poses):
        state = rng.integers(1, 3, (1, frows, fcols)).astype(np.uint8)
        want = _both_culls(sv, eng, state, pose[None], frame, words, L0, S0, seq0=9, what=(name, k))
        touched += bool((want["last_seen"] == 9).any())
    assert 3 <= touched < len(poses)
    many = mc.geometry_batch(poses)
    state = rng.integers(1, 3, (65, frows, fcols)).astype(np.uint8)
    want = _both_culls(sv, eng, state, many, frame, words, L0, S0, seq0=mc.INT_MAX - 65, what=(name, "B = 65"))
    assert (want["last_seen"] == mc.INT_MAX - 1).any()  # frame 64, the second round's first, touches


def _shape_case(sv, rows, cols):
    frame, words = SMALL["9x5"][0], dict(SMALL["9x5"][1], rows=rows, cols=cols)
    rng = np.random.default_rng(rows * 100003 + cols)
    # the vehicle over the map's first cells, turned so that the frame lies along a long map's rows or columns
    x, y = (words["top"] - 0.5) / 2.0, (words["left"] - 0.5) / 2.0
    poses = np.array([(x - 4.0, y, 1.0, 0.0), mc.FAR, (x, y, -1.0, 0.0), (x, y, 0.0, -1.0), (x - 1.3, y - 0.9, np.cos(-2.4), np.sin(-2.4))])
    state = rng.integers(0, 4, (len(poses), 9, 5)).astype(np.uint8)
    return frame, words, poses, state, rng.integers(-200, 351, (rows, cols)).astype(np.int16), rng.integers(0, 9, (rows, cols)).astype(np.int32)


def test_the_map_shapes_are_touched(sv):
    for rows, cols in [(r, c) for r in mc.MAP_ROWS for c in mc.MAP_COLS] + list(mc.LONG_MAPS):
        frame, words, poses, state, L0, S0 = _shape_case(sv, rows, cols)
        got = sv.occupancy_fuse(state, poses, frame, words, L0, S0, seq0=100)
        assert (got["last_seen"] >= 100).any(), (rows, cols)
        fresh = sv.occupancy_fuse(state, poses, frame, words, seq0=100)
        for shift in mc.map_shifts(rows, cols):
            if mc.nothing_survives(shift, rows, cols):  # 0 / -1 plus the batch
                assert _fuse_same(sv.occupancy_fuse(state, poses, frame, words, L0, S0, seq0=100, shift=shift), fresh)


def _cols_for(rows):
    return (mc.MAP_COLS if rows in mc.MAP_ROWS else ()) + tuple(c for r, c in mc.LONG_MAPS if r == rows)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", mc.MAP_ROWS + (32768,))
def test_fuse_map_shapes_and_shifts(sv, eng, rows):
    """Maps of one row, one column, one cell, around a wavefront's strip of 2 x 32 and a workgroup's tile of 8 x 32, and of 32768 cells
    along one side, under shifts that keep part of the map, its last line only, and nothing."""
    assert sorted((r, c) for r in mc.MAP_ROWS + (32768,) for c in _cols_for(r)) == sorted([(r, c) for r in mc.MAP_ROWS for c in mc.MAP_COLS] + list(mc.LONG_MAPS))
    for cols in _cols_for(rows):
        frame, words, poses, state, L0, S0 = _shape_case(sv, rows, cols)
        for shift in mc.map_shifts(rows, cols):
            _both_culls(sv, eng, state, poses, frame, words, L0, S0, seq0=100, shift=shift, what=(rows, cols, shift))


# ---------------------------------------------------------------------------------------------------------------- match

@pytest.fixture(scope="module")
def match_cases(sv):
    """name -> (grid, words, logodds, poses [3, 8, 4], the two batches of states), and the definition's results per (name, batch, w_free)."""
    cases, want = {}, {}
    for name, grid in mc.MATCH_GRIDS.items():
        words = mc.match_map(sv, grid)
        rng = np.random.default_rng(words["rows"] * 7 + words["cols"])
        logodds = rng.integers(-32768, 32768, (words["rows"], words["cols"])).astype(np.int16)
        poses = np.stack([mc.match_poses(grid), mc.match_poses(grid)[::-1], mc.match_poses(grid)])
        cases[name] = (grid, words, logodds, poses, mc.match_states(name))
        for k, state in enumerate(cases[name][4]):
            for w_occ, w_free in ((1, 0), (3, 2)):
                want[name, k, w_free] = sv.occupancy_match(state, poses, grid, words, logodds, w_occ, w_free)
    return cases, want


def test_the_match_grids_are_what_the_issue_asks_for(sv, match_cases):
    cases, want = match_cases
    assert sorted(r * c for r, c in mc.MATCH_CELLS.values()) == [4095, 4096, 4097, 8193, 3 * 4096 + 5, 65536, 65536]
    for name, (grid, words, logodds, poses, (first, second)) in cases.items():
        rows, cols = mc.MATCH_CELLS[name]
        cap = rows * cols
        assert sv.occupancy_frame_grid(grid)[3:] == (rows, cols) and first.shape == second.shape == (3, rows, cols)
        # the lists: full of occupied cells, empty, and full with both parts meeting; then full of free cells, empty, mixed
        assert mc.list_entries(first, 1) == [cap, 0, cap] and int((first[2] == 2).sum()) == cap // 2 and int((first[2] == 1).sum()) == cap - cap // 2
        assert mc.list_entries(second, 1)[:2] == [cap, 0] and mc.list_entries(second, 0)[:2] == [0, 0] and set(np.unique(second[2]).tolist()) == {0, 1, 2, 3, 255}
        # under the identity every cell lies inside the map: the counts are the lists' lengths
        a, b = want[name, 0, 2], want[name, 1, 2]
        assert a["counts"][0, 0].tolist() == [cap, 0] and a["counts"][2, 0].tolist() == [cap // 2, cap - cap // 2] and b["counts"][0, 0].tolist() == [0, cap]
        assert not want[name, 1, 0]["counts"][:2].any() and not a["counts"][1].any()
        clipped = a["counts"][0, :, 0]
        assert ((clipped > 0) & (clipped < cap)).any() and (clipped[[6, 7]] == 0).all()
    # the grids of 32768 cells in one direction carry the high bits of the packed word
    assert mc.MATCH_CELLS["long"][0] - 1 == 32767 and (mc.MATCH_CELLS["wide"][1] - 1) << 15 == 0x3FFF8000
    with pytest.raises(ValueError):
        sv.occupancy_frame_grid(dict(mc.MATCH_GRIDS["long"], x_range=(0, 32768)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(mc.MATCH_GRIDS))
def test_match_lists_across_workgroups_and_at_capacity(sv, eng, match_cases, name):
    cases, want = match_cases
    grid, words, logodds, poses, batches = cases[name]
    for k, state in enumerate(batches):
        for w_occ, w_free in ((1, 0), (3, 2)):
            entries = sum(mc.list_entries(state, w_free))
            for group in (0, 1, 8, 256):
                got, lookups = _match_counted(eng, group, lambda: _match_gpu(eng, state, poses, grid, words, logodds, w_occ, w_free))
                assert _match_same(got, want[name, k, w_free]), (name, k, w_free, group, [key for key in MATCH_KEYS if not _bits(got[key], want[name, k, w_free][key])])
                assert lookups == entries * poses.shape[1], (name, k, w_free, group)


@pytest.fixture(scope="module")
def candidates(sv):
    """(state, logodds) and per (P, placement) the poses, the index the best must have and the definition's result."""
    state, logodds = mc.candidate_case(sv)
    out = {}
    for P in mc.CANDIDATE_COUNTS + (600,):
        for placement in mc.PLACEMENTS:
            poses, at = mc.candidate_poses(P, placement)
            out[P, placement] = (poses, at, sv.occupancy_match(state, poses, mc.CANDIDATE_FRAME, mc.CANDIDATE_MAP, logodds))
    return state, logodds, out


def test_the_candidates_are_what_the_issue_asks_for(sv, candidates):
    state, logodds, cases = candidates
    assert int((state == 2).sum()) == 3 and not (state == 1).any()
    for (P, placement), (poses, at, want) in cases.items():
        assert poses.shape == (P, 4) and want["best"].tolist() == [at] and want["best_score"].tolist() == [150]
        good = want["score"][0] == 150
        assert (want["score"][0][~good] == -21).all() and (want["counts"][0, :, 0] == 3).all()
        assert np.nonzero(good)[0].tolist() == {"last": [P - 1], "first": [0], "two": [300, P - 2], "everywhere": list(range(P))}[placement]
        assert placement != "two" or (P - 2) // 256 != 300 // 256


@pytest.mark.gpu
@pytest.mark.parametrize("P", mc.CANDIDATE_COUNTS)
def test_match_many_candidates(sv, eng, candidates, P):
    """A forced group of 1 asks for P partial maxima per frame; the host widens the group until 2048 are enough (to 2, 4 and 32 for
    these P), and the automatic choice is widened the same way.  Each placement of the best in a run of its own, then all four as one
    batch - where frame 0's last pair and frame 1's first would share a slot if the partials of a frame ran past 2048."""
    state, logodds, cases = candidates
    for group in (1, 0):
        for placement in mc.PLACEMENTS:
            poses, at, want = cases[P, placement]
            got, lookups = _match_counted(eng, group, lambda: _match_gpu(eng, state, poses, mc.CANDIDATE_FRAME, mc.CANDIDATE_MAP, logodds))
            assert _match_same(got, want) and got["best"].tolist() == [at], (P, group, placement, got["best"].tolist())
            assert lookups == 3 * P
        batch = np.stack([cases[P, placement][0] for placement in mc.PLACEMENTS])
        got, lookups = _match_counted(eng, group, lambda: _match_gpu(eng, np.stack([state] * 4), batch, mc.CANDIDATE_FRAME, mc.CANDIDATE_MAP, logodds))
        assert all(_bits(got[k], np.concatenate([cases[P, placement][2][k] for placement in mc.PLACEMENTS])) for k in MATCH_KEYS), (P, group)
        assert got["best"].tolist() == [P - 1, 0, 300, 0] and lookups == 4 * 3 * P


@pytest.mark.gpu
def test_match_automatic_group_above_one(sv, eng, candidates):
    """Batch 4 with P = 600 and the automatic choice.  map_match.cpp takes the largest k in 8 .. 1 with batch x ceil(P / 2^k) >= 1024:
    4 x ceil(600 / 4) = 600 misses, 4 x ceil(600 / 2) = 1200 passes, so k = 1 and a workgroup scores G = 2 candidates (300 workgroups per
    frame, no widening).  The choice cannot be read back: the results and the counter are what is asserted."""
    state, logodds, cases = candidates
    batch = np.stack([cases[600, placement][0] for placement in mc.PLACEMENTS])
    assert 4 * ((600 + 1) // 2) >= 1024 > 4 * ((600 + 3) // 4)
    got, lookups = _match_counted(eng, 0, lambda: _match_gpu(eng, np.stack([state] * 4), batch, mc.CANDIDATE_FRAME, mc.CANDIDATE_MAP, logodds))
    assert all(_bits(got[k], np.concatenate([cases[600, placement][2][k] for placement in mc.PLACEMENTS])) for k in MATCH_KEYS)
    assert got["best"].tolist() == [599, 0, 300, 0] and lookups == 4 * 3 * 600


@pytest.mark.parametrize("fill", [32767, -32768])
def test_the_saturated_sums_are_what_the_issue_asks_for(sv, fill):
    grid, words, state, poses = mc.saturated_case(sv)
    want = sv.occupancy_match(state, poses, grid, words, np.full((words["rows"], words["cols"]), fill, np.int16), 32767, 32767)
    assert mc.list_entries(state, 1) == [4 * 1024 + 1] * 2 and poses.shape == (2, 257, 4)
    assert (want["counts"][0] == [4097, 0]).all() and (want["counts"][1] == [0, 4097]).all()  # inside the map under every candidate
    assert (want["sums"][0] == [4097 * fill, 0]).all() and (want["sums"][1] == [0, 4097 * fill]).all() and abs(1024 * fill) < 2 ** 31 < abs(4097 * fill) * 32767
    assert want["best"].tolist() == [0, 0] and want["best_score"].tolist() == [32767 * 4097 * fill, -32767 * 4097 * fill]


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [32767, -32768])
def test_match_sums_at_the_ends_of_int16(sv, eng, fill):
    """A little over four staged chunks of the same extreme word: with G = 256 one lane sums each chunk of 1024 alone, in int32."""
    grid, words, state, poses = mc.saturated_case(sv)
    logodds = np.full((words["rows"], words["cols"]), fill, np.int16)
    want = sv.occupancy_match(state, poses, grid, words, logodds, 32767, 32767)
    for group in (256, 1, 0):
        got, lookups = _match_counted(eng, group, lambda: _match_gpu(eng, state, poses, grid, words, logodds, 32767, 32767))
        assert _match_same(got, want), (fill, group, [k for k in MATCH_KEYS if not _bits(got[k], want[k])])
        assert lookups == 2 * 4097 * 257


# ---------------------------------------------------------------------------------------------------------------- paths

def _key(words):
    return tuple(sorted(words.items()))


@pytest.mark.parametrize("n_discs", [64, 63])
@pytest.mark.parametrize("map_name", ["plain"])
def test_the_long_paths_are_what_the_issue_asks_for(sv, map_name, n_discs):
    """On the definition: path 0's only hit is its last step's last disc, path 1's only hit is step 0's disc 0, path 2 has none."""
    T = mc.LONG_STEPS
    words, d2, paths, centres, r2 = mc.long_paths(sv, n_discs, _key(_small_words(sv, map_name)))
    assert paths.shape == (3, T, 4) and T == 65535 and len(centres) == n_discs and 64 % n_discs == (0 if n_discs == 64 else 1)
    for k, only in ((0, (T - 1, n_discs - 1)), (1, (0, 0)), (2, None)):
        inside, r, c = sv.clearance_cells(words, paths[k], centres)
        hits = np.argwhere(inside & (d2[r, c] <= r2))
        assert inside.all() and hits.tolist() == ([list(only)] if only else []), (k, hits[:4].tolist())
    want = mc.long_paths_definition(sv, n_discs, _key(words))
    assert want["first_hit"].tolist() == [T - 1, 0, T] and want["min_d2"].tolist() == [81, 0, F] and want["n_outside"].tolist() == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_discs", [64, 63])
def test_paths_of_the_most_steps(sv, eng, n_discs):
    """65535 steps x 64 discs, the entry's stated maximum, and x 63, where a lane's disc index wraps on almost every round."""
    words, d2, paths, centres, r2 = mc.long_paths(sv, n_discs, _key(_small_words(sv, "plain")))
    want = mc.long_paths_definition(sv, n_discs, _key(words))
    got = _paths_gpu(eng, _cuda(d2), words, paths, centres, r2, mc.LONG_R)
    assert all(_bits(got[k], want[k]) for k in PATH_KEYS), {k: (got[k].tolist(), want[k].tolist()) for k in PATH_KEYS}


@pytest.mark.gpu
@pytest.mark.parametrize("n_discs", mc.PATH_DISCS)
@pytest.mark.parametrize("map_name", sorted(SMALL_MAPS))
def test_paths_with_disc_counts_that_do_not_divide_64(sv, eng, map_name, n_discs):
    """The field and the discs of test_clearance.py's test_paths_equal_the_definition: step_q = 32, 12, 1, 1 and step_r = 0, 4, 31, 1."""
    words = _small_words(sv, map_name)
    rng = np.random.default_rng(500 + n_discs)
    R = 9
    d2 = rng.choice(np.array([0, 1, 2, 50, 81, F], np.uint16), (160, 160), p=[0.02, 0.02, 0.02, 0.04, 0.1, 0.8])
    t_d2 = _cuda(d2)
    centres = np.round(rng.uniform(-3.0, 3.0, (n_discs, 2)) * 8) / 8
    r2 = rng.choice(np.array([0, 1, 49, 80, 81], np.int32), n_discs)
    r2[0], r2[-1] = 0, 81
    hits = clipped = 0
    for K in PATH_COUNTS:
        for T in mc.PATH_STEPS:
            poses = _poses_around(sv, rng, words, K * T).reshape(K, T, 4)
            want = sv.clearance_paths(d2, words, poses, centres, r2, R)
            got = _paths_gpu(eng, t_d2, words, poses, centres, r2, R)
            assert all(_bits(got[k], want[k]) for k in PATH_KEYS), (map_name, n_discs, K, T, [k for k in PATH_KEYS if not _bits(got[k], want[k])])
            hits += int(((want["first_hit"] > 0) & (want["first_hit"] < T)).sum())
            clipped += int(((want["n_outside"] > 0) & (want["n_outside"] < T * n_discs)).sum())
    assert hits > 0 and clipped > 0
    # a hit at the very last lookup and one at the very first, as in test_paths_equal_the_definition
    T = 65
    poses = _poses_around(sv, rng, words, 3 * T)[:T]
    ok, r, c = sv.clearance_cells(words, poses, centres)
    assert ok.all()
    paths = np.stack([poses, poses[::-1], poses])
    far = np.full((160, 160), F, np.uint16)
    far[r[T - 1, -1], c[T - 1, -1]] = r2[-1]
    want = sv.clearance_paths(far, words, paths, centres, r2, R)
    assert want["first_hit"].tolist() == [T - 1, 0, T - 1]
    got = _paths_gpu(eng, _cuda(far), words, paths, centres, r2, R)
    assert all(_bits(got[k], want[k]) for k in PATH_KEYS)
