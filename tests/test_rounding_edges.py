"""The double-precision cell rules of the stages, each on inputs where ONE rounding decides the integer (tests/rounding_cases.py): a pose
or Q applied to a point, a division by a cell size or a depth, a floor(v + 0.5).  Random inputs cannot show a contracted multiply-add, a
division turned into a multiplication by the reciprocal or a reassociated sum - about one flip in 10^13 draws -, so a compiler flag, a
compiler upgrade or a strength reduction in one .hip file would pass every other module.

The CPU tests hold of every corpus that the package's numpy definition gives the scalar model's integers on every input, that every
mistake that applies to a front is discriminated by at least 32 inputs, and that the mistakes that cannot matter do not.  The GPU tests
run every corpus through every translation unit that compiles its front - contraction and division lowering are decided per .hip file -
and compare every output with the numpy definition: shape, dtype, bits, no tolerance."""
import numpy as np
import pytest

import rounding_cases as rc
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_clearance import PATH_KEYS, _paths_gpu
from test_flow import _gpu_match
from test_warp import _gpu as _warp_gpu
from warp_cases import same as _warp_same
from flow_cases import same as flow_same
from test_map_match import _gpu as _flat_match_gpu, _same as _flat_match_same
from test_occupancy_map import _gpu as _fuse_gpu, _same as _fuse_same
from test_occupancy import _bits, _check as _occupancy_check
from test_top_view import _d1_points
from test_voxel_cloud import _check as _cloud_check
from test_voxel_flatten import _differ as _flatten_differ, _host as _flatten_host
from test_voxel_render import _differ as _render_differ, _engine_render, _host as _render_host
from test_voxel_map import _engine_map, _host as _map_host, _same as _map_same
from test_voxel_match import _gpu as _match_gpu
from test_voxel_align import _gpu as _align_gpu
from test_voxel_normals import _planes_on_device
from test_voxel_carve import _engine_carve, _same_arrays, _touched
from voxel_align_cases import same as align_same
from voxel_carve_cases import STATS as CARVE_STATS
from voxel_match_cases import same as match_same

AT_LEAST = 32  # inputs per (front, mistake)


def _enough(corpus, mistakes, none=()):
    counts = rc.counts_of(corpus, mistakes)
    assert all(counts[m] >= AT_LEAST for m in mistakes if m not in none), counts
    assert all(counts[m] == 0 for m in none), counts
    assert 0 < len(corpus) < 4096  # below sites()' limit: nothing was cut
    return counts


# ---------------------------------------------------------------------------------------------------------------- the voxel map's cell

def _voxel_key(r):
    return r[0] | r[1] << 20 | r[2] << 40


@pytest.fixture(scope="module")
def voxel(sv):
    """The corpus by frames, the map of its rows alone, the dense map, and the definition's answers: computed once."""
    corpus = rc.voxel_corpus()
    xyz, counts, poses, where = rc.frames_of(corpus)
    call = (xyz, None, None, counts, poses)
    alone = sv.voxel_map_insert(sv.voxel_map_state(sv.voxel_map_params(**rc.VOXEL_BOX)), *call)
    fill = rc.voxel_fill()
    dense = sv.voxel_map_insert(sv.voxel_map_state(sv.voxel_map_params(**rc.VOXEL_BOX)), *fill)
    return dict(corpus=corpus, call=call, where=where, alone=alone, fill=fill, dense=dense)


def test_voxel_corpus(sv, voxel):
    """Every input of the corpus lands, in voxel_map_insert, voxel_map_match and voxel_map_align_sums, in the model's cell at the model's
    offset; every mistake moves at least 32 rows into another cell or to another offset."""
    corpus, model = voxel["corpus"], rc.VoxelCell()
    _enough(corpus, rc.VOXEL_MISTAKES)
    assert model.cells == list(voxel["alone"]["params"]["cells"])
    want = [model.result(inp, rc.DEFINITION) for inp, _ in corpus]
    n, S = {}, {}
    for r in want:
        k = _voxel_key(r)
        n[k] = n.get(k, 0) + 1
        S[k] = [a + b for a, b in zip(S.get(k, (0, 0, 0)), r[3:])]
    alone = voxel["alone"]
    assert alone["dropped"] == 0 and alone["key"].tolist() == sorted(n) and alone["n"].tolist() == [n[k] for k in sorted(n)]
    assert alone["S"].tolist() == [S[k] for k in sorted(n)]
    # row by row: voxel_map_align_sums' pair of a row in a map that holds the corpus' own voxels is the row's own cell unless a neighbour's
    # mean lies nearer, and voxel_map_match's inside / hits count every row
    xyz, _, _, counts, poses = voxel["call"]
    got = sv.voxel_map_match(alone, xyz, None, counts, poses[:, None, :])
    assert got["inside"][:, 0].tolist() == counts.tolist() and got["hits"][:, 0].tolist() == counts.tolist()
    mean = {k: [s // n[k] for s in S[k]] for k in n}
    d2 = np.zeros(rc.FRAMES, np.int64)
    for (b, _), r in zip(voxel["where"], want):
        d2[b] += sum((u - m) ** 2 for u, m in zip(r[3:], mean[_voxel_key(r)]))
    assert got["d2"][:, 0].tolist() == d2.tolist()
    # a mistake moves the row: the frame's d2 against the corpus' own means changes in every frame that holds a discriminating row
    for name in rc.VOXEL_MISTAKES:
        ops, moved, changed = rc.mistake(name), 0, np.zeros(rc.FRAMES, np.int64)
        for (b, _), (inp, tags), r in zip(voxel["where"], corpus, want):
            bad = model.result(inp, ops)
            assert (bad != r) == (name in tags)
            if bad != r:
                moved += 1
                own = mean.get(_voxel_key(bad))
                changed[b] += 1 if own is None else abs(sum((u - m) ** 2 for u, m in zip(bad[3:], own)) - sum((u - m) ** 2 for u, m in zip(r[3:], mean[_voxel_key(r)])))
        assert moved >= AT_LEAST and (changed > 0).sum() >= min(AT_LEAST, rc.FRAMES // 2), (name, moved)


def _unit_voxel_map(sv, eng, voxel):
    buf, words = _engine_map(eng, sv, rc.VOXEL_BOX, [voxel["call"]])
    assert _map_same(_map_host(eng.voxel_map_rows(buf, words, dtype="f64")), sv.voxel_map_rows(voxel["alone"], dtype="f64"))
    assert eng.voxel_map_stats(buf) == (len(voxel["alone"]["key"]), 0, False)


def _unit_voxel_match(sv, eng, voxel):
    xyz, _, _, counts, poses = voxel["call"]
    for calls, state in (([voxel["call"]], voxel["alone"]), ([voxel["fill"]], voxel["dense"])):
        buf, words = _engine_map(eng, sv, rc.VOXEL_BOX, calls)
        assert match_same(_match_gpu(eng, buf, words, xyz, None, counts, poses[:, None, :]), sv.voxel_map_match(state, xyz, None, counts, poses[:, None, :]))


def _unit_voxel_align(sv, eng, voxel):
    xyz, _, _, counts, poses = voxel["call"]
    buf, words = _engine_map(eng, sv, rc.VOXEL_BOX, [voxel["fill"]])
    origin = sv.voxel_align_origin(words, poses)
    want = sv.voxel_map_align_sums(voxel["dense"], xyz, None, counts, poses, origin)
    assert (want["sums"][:, 0] == counts).all() and (want["sums"][:, 1] > 0).any()
    assert align_same(_align_gpu(eng, buf, words, (xyz, None, counts), poses, origin), want)


def _unit_voxel_normal(sv, eng, voxel):
    xyz, _, _, counts, poses = voxel["call"]
    buf, words = _engine_map(eng, sv, rc.VOXEL_BOX, [voxel["fill"]])
    dirs = sv.voxel_normal_dirs()
    normal = (np.arange(len(voxel["dense"]["key"])) % len(dirs)).astype(np.int32)  # the stage takes the words as they are
    got = _planes_on_device(eng, sv, buf, words, voxel["dense"], (xyz, None, counts), poses, sv.voxel_align_origin(words, poses), normal, dirs)
    assert (got["sums"][:, 2] > 0).any()


def _unit_voxel_carve(sv, eng, voxel):
    xyz, _, _, counts, poses = voxel["call"]
    buf, words = _engine_map(eng, sv, rc.VOXEL_BOX, [voxel["fill"]])
    case = dict(frames=(xyz, None, counts, poses), kw=dict(origin=(0.0, 0.0, 0.0), seq0=1, margin=0))
    state = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in voxel["dense"].items()}
    want = sv.voxel_map_carve(state, xyz, None, counts, poses, apply=False, **case["kw"])
    assert want["rays"] == counts.sum() and want["touched"] > 100
    res = _engine_carve(eng, buf, words, case, apply=False)
    assert res.stats.cpu().tolist() == [want[k] for k in CARVE_STATS]
    key, miss = _touched(eng, buf, words, res)
    assert _same_arrays(key, want["key"]) and _same_arrays(miss, want["miss"])


# ---------------------------------------------------------------------------------------------------------------- the reprojected pixel

def _grid_cell(sv, inp):
    """(row, col) of the one occupied cell of the top view of an input."""
    d, Q, XR, XT = rc.reproject_call(inp)
    g = sv.points_2_top_view(_d1_points(d, Q, XR, XT)[0], mode="count", **rc.GRID)
    assert g.sum() == 1
    return tuple(int(v[0]) for v in np.nonzero(g))


def test_reprojected_corpora(sv):
    """The one valid pixel of every input lies, by points_2_top_view, occupancy_grid and voxel_cloud, where the model puts it."""
    grid, cloud = rc.reproject_corpus("grid"), rc.reproject_corpus("cloud")
    _enough(grid, rc.REPROJECT_MISTAKES)
    _enough(cloud, rc.CLOUD_MISTAKES)
    model = rc.Reprojected("grid")
    for inp, tags in grid:
        want = model.result(inp, rc.DEFINITION)
        assert _grid_cell(sv, inp) == want
        d, Q, XR, XT = rc.reproject_call(inp)
        occ = sv.occupancy_grid(d[0], *_occupancy_rest(), Q, XR=XR, XT=XT, **rc.GRID)
        assert tuple(int(v[0]) for v in np.nonzero(occ["cells"][..., 1])) == want
        assert all((model.result(inp, rc.mistake(m)) != want) == (m in tags) for m in rc.REPROJECT_MISTAKES)
    model = rc.Reprojected("cloud")
    for inp, tags in cloud:
        want = model.result(inp, rc.DEFINITION)
        d, Q, XR, XT = rc.reproject_call(inp)
        xyz, _, cell, n, first, count = sv.voxel_cloud(d, Q, XR=XR, XT=XT, dtype="f64", **rc.CLOUD_BOX)[0]
        assert count == 1 and cell[0].tolist() == list(want[0::2]) and first[0] == inp["j"] * rc.REPROJECT_SHAPE[1] + inp["i"]
        lo, size = rc.CLOUD_BOX["lo"], rc.CLOUD_BOX["size"]
        assert xyz[0].tolist() == [lo[k] + (want[2 * k] + (want[2 * k + 1] + 0.5) / 65536.0) * size for k in range(3)]  # the offsets
        assert all((model.result(inp, rc.mistake(m)) != want) == (m in tags) for m in rc.CLOUD_MISTAKES)


def _occupancy_rest():
    """labels (every pixel an obstacle), free_row (no ray) and free_disp of the reprojection corpus' images."""
    H, W = rc.REPROJECT_SHAPE
    return np.full((H, W), 2, np.uint8), np.full(W, -1, np.int32), np.zeros(W, np.float32)


def _unit_top_view(sv, eng, reprojected):
    for d, Q, XR, XT in reprojected["grid"]:
        g = rc.GRID
        for mode in ("count", "reference"):
            got = eng.top_view_from_disparity(_cuda(d), Q, g["x_range"], g["y_range"], g["z_range"], g["scale"], XR=XR, XT=XT, disparity="d1", mode=mode).cpu().numpy()
            assert _bits(got[0], sv.points_2_top_view(_d1_points(d, Q, XR, XT)[0], mode=mode, **g))


def _unit_occupancy(sv, eng, reprojected):
    lab, row, dsp = _occupancy_rest()
    for d, Q, XR, XT in reprojected["grid"]:
        _occupancy_check(sv, eng, d, lab[None], row[None], dsp[None], Q, XR, XT, **rc.GRID)


def _unit_voxel_cloud(sv, eng, reprojected):
    for d, Q, XR, XT in reprojected["cloud"]:
        for dtype in ("f32", "f64"):
            assert _cloud_check(sv, eng, d, Q, XR=XR, XT=XT, dtype=dtype, **rc.CLOUD_BOX).tolist() == [1]


@pytest.fixture(scope="module")
def reprojected():
    """The calls (d, Q, XR, XT) of the two corpora, an input each."""
    return dict(grid=[rc.reproject_call(inp) for inp, _ in rc.reproject_corpus("grid")], cloud=[rc.reproject_call(inp) for inp, _ in rc.reproject_corpus("cloud")])


# ---------------------------------------------------------------------------------------------------------------- the flat map's cell

@pytest.fixture(scope="module")
def flat(sv):
    """The three corpora as calls and the definition's answers."""
    words = sv.occupancy_map_params(**rc.FLAT_MAP)
    logodds, d2 = rc.unique_cells(words["rows"], words["cols"], np.int16), rc.unique_cells(words["rows"], words["cols"], np.uint16)
    state, poses, where = rc.flat_match_call(rc.match_corpus())
    paths = np.array([rc.pose4(inp) for inp, _ in rc.clearance_corpus()])[:, None, :]
    disc = (np.array([rc.DISC]), np.array([0], np.int32))
    fwords = sv.occupancy_map_params(**rc.FUSE_MAP)
    fposes = np.array([rc.pose4(inp) for inp, _ in rc.fuse_corpus()])
    fstate = rc.fuse_state(len(fposes))
    return dict(words=words, logodds=logodds, d2=d2, state=state, poses=poses, where=where, paths=paths, disc=disc, fwords=fwords, fposes=fposes, fstate=fstate,
                match=sv.occupancy_match(state, poses, rc.FLAT_FRAME, words, logodds), path=sv.clearance_paths(d2, words, paths, *disc, 1),
                fuse=sv.occupancy_fuse(fstate, fposes, rc.FLAT_FRAME, fwords))


def test_flat_corpora(sv, flat):
    """occupancy_match's sum and clearance_paths' min_d2 over fields that name their cells, and occupancy_fuse's log-odds under a chequerboard
    of states, are the model's cell on every input; every mistake reads another cell on at least 32."""
    model, cols = rc.FlatCell(), flat["words"]["cols"]
    for corpus in (rc.match_corpus(), rc.clearance_corpus(), rc.fuse_corpus()):
        _enough(corpus, rc.FLAT_MISTAKES)
    assert (flat["match"]["counts"][..., 0] == 1).all()
    for (inp, tags), (b, p) in zip(rc.match_corpus(), flat["where"]):
        r, c = model.result(inp, rc.DEFINITION)
        assert flat["match"]["sums"][b, p, 0] == flat["logodds"][r, c]
        assert all((flat["logodds"][model.result(inp, rc.mistake(m))] != flat["logodds"][r, c]) == (m in tags) for m in rc.FLAT_MISTAKES)
    assert not flat["path"]["n_outside"].any()
    for k, (inp, tags) in enumerate(rc.clearance_corpus()):
        r, c = model.result(inp, rc.DEFINITION)
        assert flat["path"]["min_d2"][k] == r * cols + c
        assert all((model.result(inp, rc.mistake(m)) != (r, c)) == (m in tags) for m in rc.FLAT_MISTAKES)
    back, w = rc.FuseBack(), flat["fwords"]
    for b, (inp, tags) in enumerate(rc.fuse_corpus()):
        fr, fc = back.result(inp, rc.DEFINITION)
        alone = sv.occupancy_fuse(flat["fstate"][b], flat["fposes"][b], rc.FLAT_FRAME, w)
        assert alone["logodds"][inp["r"], inp["col"]] == (w["l_occ"] if flat["fstate"][b, fr, fc] == 2 else -w["l_free"])
        for m in rc.FLAT_MISTAKES:  # one cell off on one axis: the other state
            bad = back.result(inp, rc.mistake(m))
            assert (bad != (fr, fc)) == (m in tags) and (bad == (fr, fc) or flat["fstate"][b][bad] != flat["fstate"][b, fr, fc])
    assert np.abs(flat["fuse"]["logodds"]).max() < 32767


def _unit_map_match(sv, eng, flat):
    assert _flat_match_same(_flat_match_gpu(eng, flat["state"], flat["poses"], rc.FLAT_FRAME, flat["words"], flat["logodds"]), flat["match"])


def _unit_clearance(sv, eng, flat):
    got = _paths_gpu(eng, _cuda(flat["d2"]), flat["words"], flat["paths"], *flat["disc"], 1)
    assert all(_bits(got[k], flat["path"][k]) for k in PATH_KEYS)


def _unit_occupancy_map(sv, eng, flat):
    assert _fuse_same(_fuse_gpu(eng, flat["fstate"], flat["fposes"], rc.FLAT_FRAME, flat["fwords"]), flat["fuse"])


# ---------------------------------------------------------------------------------------------------------------- the moved pixel

@pytest.fixture(scope="module")
def moved(sv):
    """The three corpora as calls, and the definition's answers."""
    d, poses = rc.warp_call(rc.moved_corpus("warp"))
    de, pe = rc.warp_call(rc.edge_corpus())
    matches, counts, mposes = rc.sums_call(rc.moved_corpus("sums"))
    prev, cur, dm, guess = rc.match_call(rc.moved_corpus("match"))
    return dict(warp=(d, poses), edge=(de, pe), sums=(matches, counts, mposes), match=(prev, cur, dm, guess),
                warped=sv.disparity_warp(d, None, rc.MOVED_CAM, poses), edged=sv.disparity_warp(de, None, rc.EDGE_CAM, pe),
                summed=sv.flow_pose_sums(matches, counts, rc.MOVED_CAM, mposes), matched=sv.flow_match(prev, cur, dm, None, rc.MOVED_CAM, guess, **rc.MATCH_WORDS))


def _covered(expected):
    return (int(expected.max()),) + tuple(zip(*(v.tolist() for v in np.nonzero(expected))))


def test_moved_corpora(sv, moved):
    """disparity_warp's expected map, flow_pose_sums' E and Ed and flow_match's row are the model's on every input; every mistake changes
    them on at least 32; a fused 16 q + 0.5 - and for the matcher, which does not use it, fb / z - on none."""
    assert rc.moved_camera() == {k: v for k, v in sv.flow_camera(rc.MOVED_CAM).items() if k != "b"}
    for kind in ("warp", "sums", "match"):
        _enough(rc.moved_corpus(kind), rc.moved_mistakes(kind) + rc.moved_none(kind), rc.moved_none(kind))
    model = rc.Moved("warp")
    for b, (inp, tags) in enumerate(rc.moved_corpus("warp")):
        want = model.result(inp, rc.DEFINITION)
        assert (_covered(moved["warped"]["expected"][b]) if len(want) > 1 else (want[0],)) == want, b
    # exact halves, negative values, and 0.5 - 2^-54, whose sum with 0.5 rounds up to 1: column 1 by the definition, column 0 by rint
    edge, model = rc.edge_corpus(), rc.Moved("warp", rc.EDGE_CAM)
    assert len(edge) >= 8 and all("half:rint" in tags and model.values(inp, rc.DEFINITION)[0] == rc.ROUNDS_UP for inp, tags in edge)
    for b, (inp, tags) in enumerate(edge):
        want = model.result(inp, rc.DEFINITION)
        assert _covered(moved["edged"]["expected"][b]) == want and all(c >= 1 for _, c in want[1:]) and any(c == 0 for _, c in model.result(inp, rc.mistake("half:rint"))[1:])
    values = [rc.Moved("warp").values(inp, rc.DEFINITION)[inp["axis"]] for inp, tags in rc.moved_corpus("warp") if "half:rint" in tags]
    assert sum(v % 1.0 == 0.5 for v in values) >= AT_LEAST and sum(v < 0 for inp, _ in rc.moved_corpus("warp") for v in rc.Moved("warp").values(inp, rc.DEFINITION)[:2]) >= AT_LEAST
    model, (matches, _, _) = rc.Moved("sums"), moved["sums"]
    for b, (inp, tags) in enumerate(rc.moved_corpus("sums")):
        pu, pv, pd = model.result(inp, rc.DEFINITION)
        ru, rv, rd = 16 * int(matches[b, 0, 3]) - pu, 16 * int(matches[b, 0, 4]) - pv, int(matches[b, 0, 5]) - pd
        assert moved["summed"][b, :5].tolist() == [1, 1, 1, ru * ru + rv * rv, rd * rd] and abs(ru) <= 8 and abs(rv) <= 8 and rd == 1, b
    model, got = rc.Moved("match"), moved["matched"]
    for b, (inp, tags) in enumerate(rc.moved_corpus("match")):
        want = model.result(inp, rc.DEFINITION)
        row = () if got["counts"][b] == 0 else tuple(got["matches"][b, 0, 3:5].tolist() + got["cost"][b, 0].tolist())
        assert row == want and got["counts"][b] in (0, 1), b
    assert (got["counts"] == 1).sum() >= len(got["counts"]) // 4


def _unit_warp(sv, eng, moved):
    for corpus, want, cam in (("warp", "warped", rc.MOVED_CAM), ("edge", "edged", rc.EDGE_CAM)):
        d, poses = moved[corpus]
        assert _warp_same(_warp_gpu(eng, d, None, cam, poses), moved[want])


def _unit_flow(sv, eng, moved):
    prev, cur, dm, guess = moved["match"]
    assert flow_same(_gpu_match(eng, prev, cur, dm, None, rc.MOVED_CAM, guess, **rc.MATCH_WORDS), moved["matched"])
    matches, counts, poses = moved["sums"]
    got = eng.flow_pose_sums(_cuda(matches), _cuda(counts), rc.MOVED_CAM, poses).cpu().numpy()
    assert _bits(got, moved["summed"])


# ---------------------------------------------------------------------------------------------------------------- the rendered and the flattened voxel

def _one_voxel(sv, box, call):
    return sv.voxel_map_insert(sv.voxel_map_state(sv.voxel_map_params(**box)), *call)


@pytest.fixture(scope="module")
def rendered(sv):
    """Per map of the render corpus a case as test_voxel_render takes it, the indices of its inputs and the definition's images."""
    out = []
    for call, cams, at in rc.render_calls(rc.render_corpus()):
        case = dict(params=rc.VOXEL_BOX, calls=[call], cams=cams, camera=rc.RENDER_CAM, measured=None, kw=dict(r_max=rc.R_MAX))
        out.append((case, at, sv.voxel_map_render(_one_voxel(sv, rc.VOXEL_BOX, call), cams, rc.RENDER_CAM, r_max=rc.R_MAX)))
    return out


@pytest.fixture(scope="module")
def flattened(sv):
    """Per input of the flatten corpus a case as test_voxel_flatten takes it and the definition's outputs."""
    flat, out = sv.occupancy_map_params(**rc.FLATTEN_MAP), []
    for inp, _ in rc.flatten_corpus():
        box = rc.flatten_box(inp)
        call = rc.centre_call(box["lo"], inp["rels"])
        case = dict(params=box, calls=[call], flat=flat, spec=sv.voxel_flatten_params(sv.voxel_map_params(**box)), kw={})
        out.append((case, sv.voxel_map_flatten(_one_voxel(sv, box, call), flat, case["spec"])))
    return out


def test_centre_corpora(sv, rendered, flattened):
    """voxel_map_render's depth image of a view and voxel_map_flatten's cell counts are the model's square, depth and flat cell on every
    input; every mistake, those of the voxel's centre included, changes them on at least 32."""
    corpus, model = rc.render_corpus(), rc.Rendered()
    _enough(corpus, rc.RENDER_MISTAKES)
    assert len(rendered) == rc.RENDER_MAPS and sorted(i for _, at, _ in rendered for i in at) == list(range(len(corpus)))
    for case, at, want in rendered:
        state = _one_voxel(sv, rc.VOXEL_BOX, case["calls"][0])
        assert len(state["key"]) == 1 and state["n"].tolist() == [sum(rc.CENTRE_WEIGHTS)] and state["dropped"] == 0
        assert sv.voxel_map_rows(state, dtype="f64")["xyz"][0].tolist() == rc.voxel_centre(model.lo, model.size, model.cells, corpus[at[0]][0]["rels"], rc.DEFINITION)
        for v, i in enumerate(at):
            zq, x0, x1, y0, y1 = model.result(corpus[i][0], rc.DEFINITION)
            ys, xs = np.nonzero(want["depth"][v] >= 0)
            assert (xs.min(), xs.max(), ys.min(), ys.max()) == (x0, x1, y0, y1) and len(xs) == (x1 - x0 + 1) * (y1 - y0 + 1) and (want["depth"][v][ys, xs] == zq).all(), i
            assert want["stats"][v].tolist() == [1, len(xs)]
    corpus, model = rc.flatten_corpus(), rc.Flattened()
    _enough(corpus, rc.CENTRE_MISTAKES)
    for (inp, tags), (case, want) in zip(corpus, flattened):
        assert want["stats"][:2].tolist() == [1, 0] and tuple(int(v[0]) for v in np.nonzero(want["cells"].sum(-1))) == model.result(inp, rc.DEFINITION)
        assert all((model.result(inp, rc.mistake(m)) != model.result(inp, rc.DEFINITION)) == (m in tags) for m in rc.CENTRE_MISTAKES)


def _unit_voxel_render(sv, eng, rendered):
    for case, _, want in rendered:
        buf, words = _engine_map(eng, sv, case["params"], case["calls"])
        assert _render_differ(_render_host(_engine_render(eng, buf, words, case)), want) == []


def _unit_voxel_flatten(sv, eng, flattened):
    for case, want in flattened:
        buf, words = _engine_map(eng, sv, case["params"], case["calls"])
        assert _flatten_differ(_flatten_host(eng.voxel_map_flatten(buf, words, case["flat"], case["spec"])), want) == []


UNITS = {
    "voxel_render_kernels": ("rendered", _unit_voxel_render),
    "voxel_flatten_kernels": ("flattened", _unit_voxel_flatten),
    "warp_kernels": ("moved", _unit_warp),
    "flow_kernels": ("moved", _unit_flow),
    "map_match_kernels": ("flat", _unit_map_match),
    "clearance_kernels": ("flat", _unit_clearance),
    "occupancy_map_kernels": ("flat", _unit_occupancy_map),
    "top_view_kernels": ("reprojected", _unit_top_view),
    "occupancy_kernels": ("reprojected", _unit_occupancy),
    "voxel_kernels": ("reprojected", _unit_voxel_cloud),
    "voxel_map_kernels": ("voxel", _unit_voxel_map),
    "voxel_match_kernels": ("voxel", _unit_voxel_match),
    "voxel_align_kernels": ("voxel", _unit_voxel_align),
    "voxel_normal_kernels": ("voxel", _unit_voxel_normal),
    "voxel_carve_kernels": ("voxel", _unit_voxel_carve),
}


@pytest.mark.gpu
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_unit_on_the_device(sv, eng, request, unit):
    front, run = UNITS[unit]
    run(sv, eng, request.getfixturevalue(front))
