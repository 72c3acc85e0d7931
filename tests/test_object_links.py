"""Object links (group (AB)): stereo_vision.sv.object_links against numbers worked out by hand on a painted case (track_cases.py) and
against its match-by-match form, a synthetic scene with a known motion, the host's ObjectTracks, and the GPU path - shape, dtype and
bits - against the numpy form."""
import ctypes
import os

import numpy as np
import pytest

import flow_cases as fc
import track_cases as tc
import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from track_cases import call, same

SV_ERR_ARG = -1
# |motion - truth| of the moving box and |motion| of the static box after the gated round, metres per frame, measured with the numpy
# definition on seeds 0 .. 3 of track_cases.moving_scene; the bounds are twice the worst seed.
MOVING_ERR = (0.00682, 0.00258, 0.00361, 0.00103)
STATIC_ERR = (0.00871, 0.00402, 0.00253, 0.00411)
MOVING_BOUND, STATIC_BOUND = 2 * max(MOVING_ERR), 2 * max(STATIC_ERR)


def _both(sv, case, **over):
    """The numpy form, after it has been held against the brute form."""
    got, want = call(sv.object_links, case, **over), call(sv.object_links_brute, case, **over)
    assert same(got, want), [(k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:5].tolist()) for k, _ in tc.FIELDS]
    return got


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_painted_by_hand(sv):
    got = _both(sv, tc.painted())
    assert got["votes"].tolist() == [tc.PAINTED_VOTES] and got["link"].tolist() == [tc.PAINTED_LINK]
    assert got["sums"][0, :, 0].tolist() == tc.PAINTED_N and got["sums"][0, :, 1].tolist() == tc.PAINTED_N and (got["sums"][0, 2] == 0).all()
    assert (got["sums"][..., 15] == 0).all()
    # match 0 alone, by hand: X0 = ((6 - 23.5) 8 / 80, (6 - 15.5) 8 / 80, 40 * 8 / 80) = (-1.75, -0.95, 4), Xc = X0 + (0.01, 0, -0.05); X1 = (-1.45, -0.85,
    # 4): m = floor(1024 (0.29, 0.1, 0.05) + 0.5) = (297, 102, 51), p = floor(1024 X1 + 0.5) = (-1485, -870, 4096)
    one = tc.painted(skip=range(1, 14))
    alone = _both(sv, one, min_votes=1)
    assert alone["link"][0, 0].tolist() == [0, 1, 1, 1] and alone["sums"][0, 0, 6:9].tolist() == [297, 102, 51] and alone["sums"][0, 0, 12:15].tolist() == [-1485, -870, 4096]
    assert alone["sums"][0, 0, 9:12].tolist() == [297 ** 2, 102 ** 2, 51 ** 2]
    mo = sv.object_motion(alone["sums"], alone["link"])
    assert np.allclose(mo["motion"][0, 0], np.array([297, 102, 51]) / 1024.0, atol=0, rtol=1e-15) and np.isnan(mo["motion"][0, 1:]).all() and mo["n"].tolist() == [[1, 0, 0]]


def test_painted_band_votes_and_share_at_their_limits(sv):
    case = tc.painted()
    assert _both(sv, case, band_q=7)["votes"].tolist() == [[[3, 3, 0, 4], [1, 1, 2, 4], [0, 0, 0, 0]]]  # matches 1 and 9 sit at a difference of 8
    links = lambda **w: _both(sv, case, **w)["link"][0, :, 0].tolist()
    assert links(min_votes=3) == [0, 2, -1] and links(min_votes=4) == [0, -1, -1] and links(min_votes=5) == [-1, -1, -1]
    assert links(share=192) == [0, 2, -1] and links(share=193) == [0, -1, -1]  # 256 * 3 = 192 * 4
    assert links(share=204) == [0, -1, -1] and links(share=205) == [-1, -1, -1]  # 256 * 4 = 1024 >= 204 * 5 = 1020, < 205 * 5
    unlinked = _both(sv, case, min_votes=4)
    assert unlinked["link"][0, 1].tolist() == [-1, 3, 4, 1] and (unlinked["sums"][0, 1] == 0).all()


def test_painted_contest_for_one_current_box(sv):
    unequal = _both(sv, tc.painted_contest((5, 7)))  # 3 votes against 4: the second box keeps it
    assert unequal["votes"].tolist() == [[[3, 0, 0, 3], [4, 0, 0, 4], [0, 0, 0, 0]]] and unequal["link"].tolist() == [[[-1, 3, 3, 0], [0, 4, 4, 0], [-1, 0, 0, 0]]]
    assert unequal["sums"][0, :, 0].tolist() == [0, 4, 0]
    equal = _both(sv, tc.painted_contest((7,)))  # 4 against 4: the lower i keeps it
    assert equal["link"].tolist() == [[[0, 4, 4, 0], [-1, 4, 4, 0], [-1, 0, 0, 0]]] and equal["sums"][0, :, 0].tolist() == [3, 0, 0]  # match 5 has no d1q


@pytest.mark.parametrize("seed", range(4))
def test_random_against_brute(sv, seed):
    case = tc.random_case(seed)
    first = _both(sv, case)
    assert (first["link"][..., 0] >= 0).sum() >= 3 and first["sums"][..., 0].sum() > 30
    centre = sv.object_centre(first["sums"])
    gated = _both(sv, case, gate_m=300, centre=centre)
    assert same({k: gated[k] for k in ("votes", "link")} | {"sums": first["sums"]}, first) and (gated["sums"][..., 1] == first["sums"][..., 1]).all()
    assert 0 < gated["sums"][..., 0].sum() < first["sums"][..., 0].sum()
    assert same(call(sv.object_links, case, gate_m=300, centre=None), first) and same(call(sv.object_links, case, gate_m=0, centre=centre), first)  # no centre or no gate: no gate
    for b in range(2):  # a frame of the batch is the frame alone
        alone = dict(case, **{k: case[k][b:b + 1] for k in tc.ORDER})
        assert same(call(sv.object_links, alone), {k: first[k][b:b + 1] for k, _ in tc.FIELDS})


def test_counts_and_shapes(sv):
    case = tc.random_case(1, n=300, B=3)
    full = call(sv.object_links, case)
    for counts, n0, n1 in (((-1, 0, 305), (-3, 99, 5), (99, -3, 7)), ((300, 300, 300), (0, 20, 1), (20, 0, 1))):
        c = dict(case, counts=np.array(counts, np.int32), n0=np.array(n0, np.int32), n1=np.array(n1, np.int32))
        got = _both(sv, c)
        clamped = dict(c, n0=np.clip(c["n0"], 0, 20).astype(np.int32), n1=np.clip(c["n1"], 0, 20).astype(np.int32), counts=np.minimum(c["counts"], 300).astype(np.int32))
        assert same(got, call(sv.object_links, clamped))
        for b in range(3):
            if counts[b] <= 0 or n0[b] <= 0:
                assert (got["votes"][b] == 0).all() and (got["link"][b] == [-1, 0, 0, 0]).all() and (got["sums"][b] == 0).all()
            a, z = min(max(n0[b], 0), 20), min(max(n1[b], 0), 20)
            assert (got["votes"][b, a:] == 0).all() and (got["votes"][b, :, z:20] == 0).all() and (got["link"][b, a:] == [-1, 0, 0, 0]).all()
    assert same(call(sv.object_links, dict(case, n0=None, n1=None)), call(sv.object_links, dict(case, n0=np.full(3, 20, np.int32), n1=np.full(3, 99, np.int32))))
    assert (full["votes"][0] != 0).any()
    none = dict(case, **{k: case[k][:, :0] for k in ("boxes0", "q0", "boxes1", "q1")})
    got = _both(sv, none)
    assert [got[k].shape for k, _ in tc.FIELDS] == [(3, 0, 1), (3, 0, 4), (3, 0, 16)]
    empty = dict(case, **{k: case[k][:0] for k in tc.ORDER})
    got = _both(sv, empty)
    assert [got[k].shape for k, _ in tc.FIELDS] == [(0, 20, 21), (0, 20, 4), (0, 20, 16)]
    for bad in (dict(band_q=-1), dict(band_q=2 ** 20 + 1), dict(min_votes=0), dict(share=257), dict(gate_m=2 ** 20 + 1), dict(gate_m=-1)):
        with pytest.raises(ValueError):
            call(sv.object_links, case, **bad)
    with pytest.raises(ValueError):
        call(sv.object_links, dict(case, boxes0=np.zeros((3, 65, 4), np.int32)))
    with pytest.raises(ValueError):
        call(sv.object_links, dict(case, width=8193))


def test_clamps(sv):
    got = _both(sv, tc.clamp_case())
    s = got["sums"][0, 0]
    assert got["link"].tolist() == [[[0, 4, 4, 0]]] and s[0] == 4 and s[1] == 4
    assert s[6:9].tolist() == [-2 * 2 ** 20, -4 * 2 ** 20, 4 * 2 ** 20] and s[9:12].tolist() == [4 * 2 ** 40] * 3  # x: three targets left of cx, one right
    assert s[12:15].tolist() == [-2 * 2 ** 30, -4 * 2 ** 30, 4 * 2 ** 30]
    for word, bad in ((9, np.nan), (11, np.nan), (0, np.inf), (10, -np.inf), (4, np.nan)):
        pose = tc.clamp_case()["poses"][0]
        pose[word] = bad
        got = _both(sv, tc.clamp_case(pose))
        assert got["link"].tolist() == [[[0, 4, 4, 0]]] and (got["sums"] == 0).all(), (word, bad)  # links from the votes, inside = 0


@pytest.mark.parametrize("seed", range(4))
def test_moving_box_in_a_static_scene(sv, seed):
    case = tc.moving_scene(seed)
    ego = sv.flow_egomotion(case["matches"], case["counts"], case["camera"])
    assert ego["ok"].all()
    case["poses"] = ego["poses"]
    got = sv.object_links_rounds(lambda gate, centre: _both(sv, case, gate_m=gate, centre=centre), tc.MOVING_GATE_M)
    assert got["link"][0, :, 0].tolist() == [0, 1] and got["centre"].shape == (1, 2, 3)
    mo = sv.object_motion(got["sums"], got["link"])
    moving = float(np.linalg.norm(mo["motion"][0, 0] - np.array(tc.MOVING_TRUTH))), float(np.linalg.norm(mo["motion"][0, 1]))
    print("seed %d: |moving - truth| %.5f m, |static| %.5f m, n %s" % (seed, moving[0], moving[1], mo["n"][0].tolist()))
    assert mo["n"][0, 0] >= 60 and mo["n"][0, 1] >= 40
    assert moving[0] <= MOVING_BOUND and moving[1] <= STATIC_BOUND
    assert np.allclose(sv.object_motion(got["sums"], got["link"], dt=0.1)["motion"], mo["motion"] * 10.0, rtol=1e-15, atol=0)


def _feed(tr, links, motions, boxes, n=None):
    """Frames of one box row each: links[k] carries frame k to k + 1."""
    out = [tr.start(boxes[0], [(0.0, 0.0, 10.0)] * len(boxes[0]))]
    for k, link in enumerate(links):
        cur = boxes[k + 1]
        out.append(tr.step(link, motions[k], [20] * len(link) if n is None else n[k], cur, [(float(j), 0.0, 10.0 + k) for j in range(len(cur))]))
    return out


def test_object_tracks_ids(sv):
    tr = sv.ObjectTracks(history=3, min_n=8, move_m=1.0, dt=0.1)
    box = lambda k: (k, k, 5, 5)
    boxes = [[box(0), box(1)], [box(2), box(3), box(4)], [box(5)], [box(6), box(7)]]
    links = [[2, 0], [-1, 0, -1], [-1]]  # frame 0: both carry on, crossed; frame 1: only its box 1 does; frame 2: the track ends
    motions = [[(0.25, 0.0, 0.0), (0.0, 0.0, 0.0625)], [(0, 0, 0), (0.5, 0.0, 0.0), (0, 0, 0)], [(0, 0, 0)]]
    f = _feed(tr, links, motions, boxes)
    assert [t["id"] for t in f[0]] == [0, 1]
    assert [t["id"] for t in f[1]] == [1, 2, 0]  # box 1 is new: the next id; ids 0 and 1 follow their links
    assert [t["id"] for t in f[2]] == [2]        # ids 0 and 1 ended, the new box of frame 1 goes on
    assert [t["id"] for t in f[3]] == [3, 4]     # nothing linked: new ids in ascending j
    assert tr.next_id == 5 and tr.frame == 3
    assert f[1][2]["motions"] == [(0.25, 0.0, 0.0)] and f[1][2]["moving"] and f[1][2]["velocity"] == pytest.approx((2.5, 0.0, 0.0)) and f[1][2]["box"] == box(4)
    assert f[1][0]["velocity"] == pytest.approx((0.0, 0.0, 0.625)) and not f[1][0]["moving"]
    assert f[1][1]["motions"] == [] and not f[1][1]["moving"] and all(v != v for v in f[1][1]["velocity"]) and f[1][1]["predicted"] == f[1][1]["pos"]
    assert f[2][0]["motions"] == [(0.5, 0.0, 0.0)] and f[2][0]["predicted"] == (0.5, 0.0, 11.0)
    with pytest.raises(ValueError):
        sv.ObjectTracks().step([0], [(0, 0, 0)], [9], [box(0)], [(0, 0, 0)])
    # two previous boxes that claim one current box: the first keeps it (object_links never says so)
    tr = sv.ObjectTracks()
    f = _feed(tr, [[0, 0]], [[(0, 0, 0), (0, 0, 0)]], [[box(0), box(1)], [box(2)]])
    assert [t["id"] for t in f[1]] == [0]


def test_object_tracks_history(sv):
    tr = sv.ObjectTracks(history=3, min_n=8, move_m=1.0, dt=0.5)
    box = (1, 2, 3, 4)
    motions = [[(0.125 * (k + 1), 0.0, -0.25)] for k in range(5)]
    n = [[20], [7], [20], [20], [20]]  # the second motion rests on too few matches: it is not kept
    f = _feed(tr, [[0]] * 5, motions, [[box]] * 6, n)
    assert [len(t[0]["motions"]) for t in f] == [0, 1, 1, 2, 3, 3] and all(t[0]["id"] == 0 for t in f)
    assert f[2][0]["n"] == 7 and f[2][0]["mean"] == f[1][0]["mean"] == (0.125, 0.0, -0.25)
    assert f[3][0]["mean"] == (0.25, 0.0, -0.25) and f[3][0]["velocity"] == (0.5, 0.0, -0.5)  # shorter than the history: the mean of two
    assert f[5][0]["motions"] == [(0.375, 0.0, -0.25), (0.5, 0.0, -0.25), (0.625, 0.0, -0.25)]  # longer: the last three
    assert f[5][0]["mean"] == (0.5, 0.0, -0.25) and f[5][0]["predicted"] == (0.5, 0.0, 13.75) and f[5][0]["velocity"] == (1.0, 0.0, -0.5)
    assert f[5][0]["moving"] and not sv.ObjectTracks(move_m=1.2, dt=0.5)._derive(dict(f[5][0]))["moving"]  # |v| = 1.118 m/s
    assert tr.lines(5, f[5]) == ["5 0 1 2 3 4 0.0 0.0 14.0 1.0 0.0 -0.5 20 1"]


def test_object_tracks_batches(sv):
    """Six frames as one batch and as 2 + 2 + 2 (each batch begins with the last frame of the one before it): the same state and lines."""
    rng = np.random.default_rng(3)
    F, M = 6, 4
    n = rng.integers(1, M + 1, F).astype(np.int32)
    tracked = dict(boxes=rng.integers(0, 100, (F, M, 4)).astype(np.int32), n=n, positions=rng.uniform(-5, 30, (F, M, 3)),
                   link=np.stack([np.concatenate([rng.permutation(M)[:, None] - 1, np.zeros((M, 3), np.int64)], 1) for _ in range(F - 1)]).astype(np.int32),
                   motion=rng.uniform(-0.3, 0.3, (F - 1, M, 3)), count=rng.integers(0, 30, (F - 1, M)))
    tracked["motion"][2, 1] = np.nan
    whole = sv.ObjectTracks()
    lines = [line for frame, rows in whole.feed(tracked) for line in whole.lines(frame, rows)]
    parts, part_lines = sv.ObjectTracks(), []
    for lo, hi in ((0, 2), (1, 4), (3, 6)):
        cut = {k: v[lo:hi] if k in ("boxes", "n", "positions") else v[lo:hi - 1] for k, v in tracked.items()}
        part_lines += [line for frame, rows in parts.feed(cut) for line in parts.lines(frame, rows)]
    state = lambda tr: [(t["id"], t["box"], t["pos"], t["motions"], t["n"]) for t in tr.tracks]
    assert lines == part_lines and len(lines) == int(n.sum()) and state(whole) == state(parts) and (whole.frame, whole.next_id) == (parts.frame, parts.next_id) == (5, whole.next_id)
    assert whole.next_id > int(n[0]) and [line.split()[0] for line in lines] == [str(k) for k in range(F) for _ in range(n[k])]


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    for name in ("sv_object_links_workspace", "sv_object_links_device", "sv_debug_object_links", "sv_track_spec"):
        assert name in text
    assert "(AB) Behind (Z)" in text and text.index("/* ---- (AA)") < text.index("/* ---- (AB)") < text.index("/* ---- (A)")
    build = util.pkg("build")
    assert "track_kernels.hip" in build.SOURCES and "track.cpp" in build.SOURCES and "track_kernels.h" in build.HEADERS
    engine = util.pkg("engine")
    assert set(engine.STAGE_SIGNATURES["track"]) == {"sv_object_links_workspace", "sv_object_links_device", "sv_debug_object_links"}
    assert ctypes.sizeof(engine.SvTrackSpec) == 6 * 8 + 16 * 4
    for argv in (["--tracks", "t.txt"], ["--batch", "2", "--tracks", "t.txt"], ["--odometry", "p.txt", "--tracks", "t.txt"]):
        with pytest.raises(SystemExit):
            sv.main(["-k", "nowhere"] + argv)
    case = tc.painted()
    got = call(engine.object_links, case)  # CPU input: the numpy form
    assert same(got, call(sv.object_links, case))
    import torch
    got = call(engine.object_links, dict(case, **{k: torch.from_numpy(case[k]) for k in tc.ORDER}))
    assert isinstance(got["votes"], np.ndarray) and same(got, call(sv.object_links, case))


# ---------------------------------------------------------------------------------------------------------------- GPU

def _gpu(eng, case, **over):
    dev = dict(case, **{k: None if case[k] is None else _cuda(case[k]) for k in tc.ORDER if k != "poses"})
    if over.get("centre") is not None:
        over = dict(over, centre=_cuda(over["centre"]))
    return {k: v.cpu().numpy() for k, v in call(eng.object_links, dev, **over).items()}


def _agree(sv, eng, case, **over):
    got, want = _gpu(eng, case, **over), call(sv.object_links, case, **over)
    assert same(got, want), [(k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:5].tolist()) for k, _ in tc.FIELDS]
    return want


@pytest.mark.gpu
def test_gpu_painted(sv, eng):
    want = _agree(sv, eng, tc.painted())
    assert want["link"].tolist() == [tc.PAINTED_LINK]
    for case in (tc.painted_contest((5, 7)), tc.painted_contest((7,))):
        _agree(sv, eng, case)
    for words in (dict(band_q=7), dict(min_votes=4), dict(share=193), dict(share=205)):
        _agree(sv, eng, tc.painted(), **words)


def _nested(n_matches, cap=None, M=64):
    """M boxes on both sides, nested about the map's middle, and matches that walk through them; match 0 is a member of all of them twice."""
    cap = n_matches if cap is None else cap
    W, H = 400, 300
    k = np.arange(M)
    boxes = np.stack([2 * k, k, W - 4 * k, H - 2 * k], 1).astype(np.int32)[None]  # box k: columns [2 k, W - 2 k), rows [k, H - k): box 63 holds (200, 150)
    i = np.arange(n_matches)
    u0 = np.where(i == 0, 200, (i * 7) % W)
    v0 = np.where(i == 0, 150, (i * 3) % H)
    m = np.full((1, cap, 6), -1, np.int32)
    m[0, :n_matches] = np.stack([u0, v0, 160 + i % 64, np.where(i == 0, 199, (u0 + 3) % W), np.where(i == 0, 149, (v0 + 1) % H), np.where(i % 9 == 5, -1, 150 + i % 50)], 1)
    q = np.where(k % 3 == 0, 0, 42).astype(np.int32)[None]
    return dict(matches=m, counts=np.array([n_matches], np.int32), poses=fc.pose_of(fc.rotation(0.002, -0.004, 0.001), (0.05, -0.02, -0.4))[None].copy(), boxes0=boxes, n0=None,
                q0=q, boxes1=boxes.copy(), n1=None, q1=q.copy(), camera=dict(fc.KITTI, width=W, height=H, cx=200.0, cy=150.0), width=W, height=H,
                words=dict(band_q=40, min_votes=1, share=0))


@pytest.mark.gpu
def test_gpu_all_64_boxes_twice(sv, eng):
    case = _nested(1)
    case["q0"][:], case["q1"][:] = 0, 0
    want = _agree(sv, eng, case)
    assert (want["votes"] == 1).all() and want["link"][0, :, 0].tolist() == [0] + [-1] * 63  # bit 63 of both words; every box wants box 0
    want = _agree(sv, eng, _nested(700))
    assert want["votes"][0, 0, 64] > 300 and want["sums"][0, :, 0].sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_gpu_chunks_turn_over(sv, eng, n):
    want = _agree(sv, eng, _nested(n, M=33))
    assert want["votes"][0, :, 33].sum() > n and want["sums"][0, :, 0].sum() > 0
    case = _nested(n, cap=n + 3, M=5)
    case["counts"][0] = n + 9  # above the capacity: the capacity; the rows behind the matches hold -1 and are skipped
    _agree(sv, eng, case)


@pytest.mark.gpu
def test_gpu_full_capacity(sv, eng):
    want = _agree(sv, eng, _nested(65536, M=64))
    assert want["votes"][0, 0, 64] > 30000 and want["sums"][0, :, 0].sum() > 1000


@pytest.mark.gpu
def test_gpu_batch_of_three(sv, eng):
    case = tc.random_case(2, n=600, B=3)
    case["counts"] = np.array([-1, 0, 600], np.int32)
    case["n0"], case["n1"] = np.array([17, 99, 9], np.int32), np.array([-3, 4, 20], np.int32)
    want = _agree(sv, eng, case, min_votes=1)
    assert (want["votes"][:2] == 0).all() and (want["link"][2, :, 0] >= 0).any()
    case["counts"] = np.array([600, 300, 605], np.int32)
    want = _agree(sv, eng, case, min_votes=1)
    assert all((want["votes"][b, :, :20] != 0).any() == (b != 0) for b in range(3)) and (want["votes"][0, :, 20] != 0).any()  # frame 0 has no current box, but members
    _agree(sv, eng, dict(case, n0=None, n1=None), min_votes=1)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_gpu_random_and_gated(sv, eng, seed):
    case = tc.random_case(seed)
    first = _agree(sv, eng, case)
    centre = sv.object_centre(first["sums"])
    _agree(sv, eng, case, gate_m=300, centre=centre)


@pytest.mark.gpu
def test_gpu_clamps(sv, eng):
    _agree(sv, eng, tc.clamp_case())
    for word, bad in ((9, np.nan), (0, np.inf), (10, -np.inf), (11, np.inf)):
        pose = tc.clamp_case()["poses"][0]
        pose[word] = bad
        _agree(sv, eng, tc.clamp_case(pose))
    for seed in range(2):
        case = tc.moving_scene(seed)
        case["poses"] = sv.flow_egomotion(case["matches"], case["counts"], case["camera"])["poses"]
        first = _agree(sv, eng, case)
        _agree(sv, eng, case, gate_m=tc.MOVING_GATE_M, centre=sv.object_centre(first["sums"]))


@pytest.mark.gpu
def test_gpu_dirty_buffers_and_two_calls(sv, eng):
    import torch
    case = tc.random_case(1, n=700)
    dev = dict(case, **{k: _cuda(case[k]) for k in tc.ORDER if k != "poses"})
    dirty = lambda shape, dtype: torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda").repeat_interleave(torch.empty((), dtype=dtype).element_size(), -1).view(dtype)
    out = {"votes": dirty((2, 20, 21), torch.int32), "link": dirty((2, 20, 4), torch.int32), "sums": dirty((2, 20, 16), torch.int64)}
    ws = dirty((2 * 700 * 2,), torch.int64)
    assert int(out["sums"][0, 0, 0]) == int.from_bytes(b"\xa5" * 8, "little", signed=True) and out["votes"].shape == (2, 20, 21)
    want = call(sv.object_links, case)
    other = call(sv.object_links, case, band_q=16, min_votes=4)
    for words, expect in (({}, want), (dict(band_q=16, min_votes=4), other), ({}, want)):  # the later calls find the earlier ones' words and sums
        res = call(eng.object_links, dev, out=out, workspace=ws, **words)
        assert res is out
        assert same({k: v.cpu().numpy() for k, v in res.items()}, expect)


@pytest.mark.gpu
def test_gpu_argument_checks(eng):
    import torch
    L = eng.track_lib()
    case = tc.painted()
    good = eng.track_spec(case["camera"], 3, 48, 32, band_q=8)
    n = 256
    buf = torch.full((12 * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # twelve regions of 1 KB
    base = buf.data_ptr()
    at = lambda k: base + 4 * n * k
    poses = torch.from_numpy(case["poses"].copy()).cuda()
    need = ctypes.c_size_t(77)

    def run(spec=good, matches=at(0), counts=at(1), pose=poses.data_ptr(), batch=1, cap=16, boxes0=at(2), n0=at(1) + 64, q0=at(3), boxes1=at(4), n1=at(1) + 128, q1=at(5),
            centre=None, votes=at(6), link=at(7), sums=at(8), ws=at(9), ws_bytes=16 * 16):
        return L.sv_object_links_device(matches, counts, pose, batch, cap, boxes0, n0, q0, boxes1, n1, q1, centre, None if spec is None else ctypes.byref(spec), votes, link, sums, ws,
                                        ws_bytes, None)

    for field, bad in (("width", 0), ("width", 8193), ("height", 0), ("height", 8193), ("max_boxes", -1), ("max_boxes", 65), ("band_q", -1), ("band_q", 2 ** 20 + 1),
                       ("min_votes", 0), ("share", -1), ("share", 257), ("gate_m", -1), ("gate_m", 2 ** 20 + 1), ("f", 0.0), ("b16", float("nan")), ("fb", -1.0), ("fb16", 0.0),
                       ("cx", float("inf")), ("cy", float("nan"))):
        spec = eng.track_spec(case["camera"], 3, 48, 32)
        setattr(spec, field, bad)
        assert run(spec=spec) == SV_ERR_ARG, field
    spec = eng.track_spec(case["camera"], 3, 48, 32)
    spec.reserved[8] = 1
    assert run(spec=spec) == SV_ERR_ARG
    for kw in (dict(spec=None), dict(matches=None), dict(counts=None), dict(pose=None), dict(boxes0=None), dict(q0=None), dict(boxes1=None), dict(q1=None), dict(votes=None),
               dict(link=None), dict(sums=None), dict(ws=None), dict(matches=at(0) + 2), dict(counts=at(1) + 1), dict(pose=poses.data_ptr() + 4), dict(boxes0=at(2) + 2),
               dict(n0=at(1) + 66), dict(q1=at(5) + 1), dict(centre=at(10) + 2), dict(votes=at(6) + 2), dict(link=at(7) + 1), dict(sums=at(8) + 4), dict(ws=at(9) + 4),
               dict(ws_bytes=16 * 16 - 1), dict(batch=-1), dict(batch=65536), dict(cap=-1), dict(cap=65537), dict(votes=at(0)), dict(link=at(2)), dict(sums=at(5)),
               dict(ws=at(0)), dict(link=at(6)), dict(sums=at(7)), dict(ws=at(8)), dict(votes=at(10), centre=at(10)), dict(sums=at(1))):
        assert run(**kw) == SV_ERR_ARG, kw
    assert eng.lib().sv_last_error(None)
    assert L.sv_object_links_workspace(16, 1, None) == SV_ERR_ARG and L.sv_object_links_workspace(-1, 1, ctypes.byref(need)) == SV_ERR_ARG
    assert L.sv_object_links_workspace(65537, 1, ctypes.byref(need)) == SV_ERR_ARG and L.sv_object_links_workspace(16, 65536, ctypes.byref(need)) == SV_ERR_ARG
    assert need.value == 77 and L.sv_object_links_workspace(16, 3, ctypes.byref(need)) == 0 and need.value == 3 * 16 * 16
    assert L.sv_debug_object_links(4) == SV_ERR_ARG and L.sv_debug_object_links(-1) == SV_ERR_ARG and L.sv_debug_object_links(0) == 0
    assert run(batch=0, matches=None, counts=None, pose=None, boxes0=None, n0=None, q0=None, boxes1=None, n1=None, q1=None, votes=None, link=None, sums=None, ws=None, ws_bytes=0) == 0
    none = eng.track_spec(case["camera"], 0, 48, 32)
    assert run(spec=none, boxes0=None, q0=None, boxes1=None, q1=None, votes=None, link=None, sums=None, ws=None) == 0  # max_boxes 0: nothing to write, no workspace used
    assert run(spec=none, ws_bytes=16 * 16 - 1) == SV_ERR_ARG  # but its size is held against the workspace call's all the same
    torch.cuda.synchronize()
    assert (buf == 0x5A5A5A5A).all()  # nothing was enqueued: no output and no byte of the workspace was touched
    for k, name in ((0, "matches"), (2, "boxes0"), (3, "q0"), (4, "boxes1"), (5, "q1")):
        flat = torch.from_numpy(case[name].reshape(-1)).cuda()
        buf[n * k:n * k + flat.numel()] = flat
    buf[n:n + 1], buf[n + 16:n + 17], buf[n + 32:n + 33] = 14, 2, 3
    assert run() == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[6 * n:6 * n + 12].reshape(3, 4).tolist() == tc.PAINTED_VOTES and got[7 * n:7 * n + 12].reshape(3, 4).tolist() == tc.PAINTED_LINK
    assert got[8 * n:8 * n + 96].view(np.int64).reshape(3, 16)[:, 0].tolist() == tc.PAINTED_N
    assert (got[6 * n + 12:7 * n] == 0x5A5A5A5A).all() and (got[7 * n + 12:8 * n] == 0x5A5A5A5A).all() and (got[8 * n + 96:9 * n] == 0x5A5A5A5A).all()  # and nothing behind them
    assert (got[9 * n:9 * n + 64] != 0x5A5A5A5A).all() and (got[9 * n + 64:] == 0x5A5A5A5A).all()


@pytest.fixture(scope="module")
def kitti_frames():
    ls = np.stack([np.repeat(util.load_png("kitti%d_left.png" % k)[..., None], 3, -1) for k in range(4)])
    rs = np.stack([np.repeat(util.load_png("kitti%d_right.png" % k)[..., None], 3, -1) for k in range(4)])
    return ls, rs


def _host_chain(sv, eng, got, camera, **words):
    """StereoRig.track's last stage through the numpy forms: CPU tensors into engine.object_links, two rounds."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a))
    bx, n, q, m, c = t(got["boxes"]), t(got["n"]), t(got["stat"])[:, :, 2].contiguous(), t(got["matches"]["matches"]), t(got["matches"]["counts"])
    used = got["rel"].copy()
    used[~got["ok"]] = np.nan
    res = sv.object_links_rounds(lambda gate, centre: eng.object_links(m, c, used, bx[:-1], n[:-1], q[:-1], bx[1:], n[1:], q[1:], camera, 1242, 375, gate_m=gate, centre=centre,
                                                                       **words), 256)
    assert isinstance(res["sums"], np.ndarray)
    return res


@pytest.mark.gpu
def test_gpu_rig_track(sv, eng, kitti_frames, tmp_path):
    import torch
    ls, rs = kitti_frames
    yml = str(tmp_path / "rectified.yml")
    with open(yml, "w") as f:
        f.write(fc.RECTIFIED_YML)
    rig = util.pkg("rig").StereoRig(1242, 375, calibration=yml, params=eng.SvParams.driver(127))
    try:
        camera = rig.render_camera(1.0)
        own = rig.track(torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda())
        objects = rig.objects(ls, rs)
        boxes = np.array([[(100, 150, 200, 120), (600, 160, 90, 60), (900, 140, 250, 200)]] * 4, np.int32)
        given = rig.track(ls, rs, boxes=boxes, n_boxes=np.array([3, 3, 2, 3], np.int32), guess=np.tile(fc.pose_of(np.eye(3), (0.0, 0.0, -1.16)), (3, 1)), min_votes=2)
        with pytest.raises(ValueError):
            rig.track(ls[:1], rs[:1])
        with pytest.raises(ValueError):
            rig.track(ls, rs, share=300)
    finally:
        rig.close()
    M = own["boxes"].shape[1]
    assert M == 64 and own["ok"].all() and own["left_out"].tolist() == np.maximum(objects.counts - 64, 0).tolist()
    assert np.array_equal(own["boxes"].cpu().numpy(), objects.boxes) and np.array_equal(own["n"].cpu().numpy(), np.minimum(objects.counts, 64))
    assert np.array_equal(own["stat"].cpu().numpy(), objects.stat) and np.array_equal(own["positions"].cpu().numpy(), objects.positions, equal_nan=True)
    want = _host_chain(sv, eng, own, camera)
    assert same({k: own[k].cpu().numpy() for k, _ in tc.FIELDS}, want) and np.array_equal(own["centre"], want["centre"])
    mo = sv.object_motion(want["sums"], want["link"])
    assert np.array_equal(own["motion"], mo["motion"], equal_nan=True) and np.array_equal(own["count"], mo["n"])
    linked = want["link"][..., 0] >= 0
    print("kitti0..3: %d of %d objects linked; motions (m/frame) %s" % (linked.sum(), own["n"].cpu().numpy()[:-1].sum(), np.round(mo["motion"][linked & (mo["n"] >= 8)], 3).tolist()))
    assert linked.sum() >= 1
    assert isinstance(given["link"], np.ndarray) and given["boxes"].shape == (4, 3, 4) and given["n"].tolist() == [3, 3, 2, 3] and given["left_out"].tolist() == [0] * 4
    want = _host_chain(sv, eng, given, camera, min_votes=2)
    assert same(given, want)
    assert (given["link"][2, 2] == [-1, 0, 0, 0]).all()  # frame 2 has two boxes


@pytest.mark.gpu
def test_gpu_cli_tracks(sv, eng, kitti_frames, tmp_path):
    from PIL import Image
    ls, rs = kitti_frames
    for sub, frames in (("image_02", ls), ("image_03", rs)):
        os.makedirs(tmp_path / "kitti" / sub)
        for i in range(4):
            Image.fromarray(frames[i]).save(tmp_path / "kitti" / sub / ("%010d.png" % i))
    poses, out, yml = str(tmp_path / "odo.txt"), str(tmp_path / "tracks.txt"), str(tmp_path / "rectified.yml")
    with open(yml, "w") as f:
        f.write(fc.RECTIFIED_YML)
    sv.main(["-k", str(tmp_path / "kitti"), "--camera_calibration", yml, "--batch", "2", "--odometry", poses, "--tracks", out])
    rig = util.pkg("rig").StereoRig(1242, 375, calibration=yml)  # the CLI's rig: the default parameters
    try:
        camera = rig.render_camera(1.0)
        got = rig.track(ls, rs)  # one batch of four, where the CLI ran (0, 1) and (1, 2, 3)
    finally:
        rig.close()
    want = _host_chain(sv, eng, got, camera)
    mo = sv.object_motion(want["sums"], want["link"])
    tracks = sv.ObjectTracks()
    lines = [line for frame, rows in tracks.feed(dict(got, link=want["link"], motion=mo["motion"], count=mo["n"])) for line in tracks.lines(frame, rows)]
    assert open(out).read() == "".join(line + "\n" for line in lines) and len(lines) == int(got["n"].sum()) > 4
    ids = [int(line.split()[1]) for line in lines]
    assert len(set(ids)) == len(ids) - int((want["link"][..., 0] >= 0).sum())  # every link carries an id into the next frame, everything else opens one
