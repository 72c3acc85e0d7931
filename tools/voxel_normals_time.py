#!/usr/bin/env python3
"""The normals of the voxel map and point-to-plane alignment on tools/voxel_align_time.py's street - about a million voxels at --size
metres, and its two frames, started 0.45 degrees and 0.7 cells off (HIP events, median of --reps calls after warm-up, min / max beside the
median; one process).  That street's blocks are poles of 3 x 3 cells, which get no normal, so the rounds and the loops are measured on a
second scene as well: the same ground with two walls along it and hollow boxes beside the middle (walled_cells).
  normals  per table (m = 16: 513 directions, m = 32: 2049): us per call of sv_voxel_normals_device into pre-allocated outputs, without and
           with `fit`, each with the pruning on and off (sv_debug_voxel_normals), timed in turns; and the directions tried - members that
           are searched x K - per microsecond.
  yardstick  the same definition with torch ops on the same device: sorted keys, 27 searchsorted look-ups with their gathers, an einsum
           over the directions, and the flattest and the widest direction by a tournament of cross-multiplied compares.  Both forms must
           agree on every normal, fit word and count before anything is timed.  Beside it the time of torch.linalg.eigh on 131072 of the same
           covariances in double - what a user would write otherwise, and no bit-exact answer.
  rounds   per frame one round of sv_voxel_plane_align_device beside one round of sv_voxel_align_device, timed in turns; with --parent-lib
           the point round of that library as well - the same call into the build of the parent commit, loaded beside this one - so that
           both builds meet the same drift of the machine.
  loops    engine.voxel_map_align to convergence with both methods at their default eps, at most 30 rounds, by the host's clock: rounds
           used, the error against the true pose, and the time; the normals' kernel is inside the plane loop's time once (fitted
           beforehand and handed over, it is not); and the planes first, then the means from where the planes ended - what a caller does
           where the planes alone leave a direction open, as on this street, whose blocks are poles of 3 x 3 cells and get no normal.
Nothing is asserted about speed.

    timeout -k 10 900 python tools/voxel_normals_time.py [--reps 21] [--parent-lib FILE.so] [--out profiles/voxel_normals_time.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_align_time as street  # noqa: E402 (the map, the frames and the timers)

PKG = street.PKG


def torch_normals(params, table, dirs, min_nb, flat, wide, chunk=32768):
    """(normal int32 [slots], fit int64 [slots,4], counts int64 [4], C float64 [M,3,3]) of the table (int64 [slots,11]) with torch ops."""
    dev = table.device
    slots = table.shape[0]
    key, n = table[:, 0], table[:, 1]
    live = ((key != -1) & (n >= 1) & (table[:, 9] >= 1) & ((table[:, 10] >> 32) >= 0)).nonzero(as_tuple=True)[0]
    e = table[live]
    vkey, by = torch.sort(e[:, 0])
    e, live = e[by], live[by]
    cell = torch.stack([(vkey >> (20 * k)) & 0xFFFFF for k in range(3)], -1)
    q = 256 * cell + (torch.div(e[:, 2:5], e[:, 1:2], rounding_mode="floor") >> 8)
    cells = torch.tensor(params["cells"], dtype=torch.int64, device=dev)
    M = vkey.numel()
    N = torch.zeros(M, dtype=torch.int64, device=dev)
    s1 = torch.zeros((M, 3), dtype=torch.int64, device=dev)
    s2 = torch.zeros((M, 3, 3), dtype=torch.int64, device=dev)
    for d in street.OFFSETS:
        cc = cell + torch.tensor(d, dtype=torch.int64, device=dev)
        on = ((cc >= 0) & (cc < cells)).all(-1)
        want = torch.where(on, cc[:, 0] | (cc[:, 1] << 20) | (cc[:, 2] << 40), torch.full_like(vkey, -2))
        at = torch.searchsorted(vkey, want).clamp(max=M - 1)
        hit = on & (vkey[at] == want)
        ev = torch.where(hit[:, None], q[at] - q, torch.zeros_like(q))
        N += hit
        s1 += ev
        s2 += ev[:, :, None] * ev[:, None, :]
    C = N[:, None, None] * s2 - s1[:, :, None] * s1[:, None, :]
    T = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
    dd = dirs[:, :3].long()
    K = dd.shape[0]
    width = 1 << (K - 1).bit_length()
    s = torch.zeros(width, dtype=torch.int64, device=dev)
    s[:K] = (dd * dd).sum(1)
    index = torch.arange(width, device=dev)
    pairs = dd[:, :, None] * dd[:, None, :]  # [K,3,3]
    best, worst, bQ, wQ, bs, ws = (torch.zeros(M, dtype=torch.int64, device=dev) for _ in range(6))
    for lo in range(0, M, chunk):
        Cc = C[lo:lo + chunk]
        m = Cc.shape[0]
        Q = torch.zeros((m, width), dtype=torch.int64, device=dev)
        for i in range(3):  # einsum("mij,kij->mk") spelled out: torch has no int64 matrix product on the device
            for j in range(3):
                Q[:, :K] += Cc[:, i, j, None] * pairs[None, :, i, j]
        for sign, into in ((1, (best, bQ, bs)), (-1, (worst, wQ, ws))):
            q_, s_, i_ = Q, s.expand(m, width), index.expand(m, width)
            w = width
            while w > 1:  # a tournament: the flattest (sign 1) or the widest (sign -1) of each pair, a tie to the lower index, s = 0 never
                h = w // 2
                qa, qb, sa, sb, ia, ib = q_[:, :h], q_[:, h:w], s_[:, :h], s_[:, h:w], i_[:, :h], i_[:, h:w]
                left, right = sign * qb * sa, sign * qa * sb
                take_b = (sb > 0) & ((sa == 0) | (left < right) | ((left == right) & (ib < ia)))
                q_, s_, i_ = torch.where(take_b, qb, qa), torch.where(take_b, sb, sa), torch.where(take_b, ib, ia)
                w = h
            into[0][lo:lo + chunk], into[1][lo:lo + chunk], into[2][lo:lo + chunk] = i_[:, 0], q_[:, 0], s_[:, 0]
    some = bs > 0
    one = torch.ones_like(bs)
    lam3 = torch.where(some, torch.div(bQ, torch.where(some, bs, one), rounding_mode="floor"), torch.zeros_like(bQ))
    lam1 = torch.where(some, torch.div(wQ, torch.where(some, ws, one), rounding_mode="floor"), torch.zeros_like(wQ))
    lam2 = T - lam1 - lam3
    given = some & (N >= min_nb) & (lam2 > 0) & (256 * lam3 <= flat * lam2) & (256 * lam2 >= wide * lam1)
    normal = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    normal[live] = torch.where(given, best, torch.full_like(best, -1)).int()
    fit = torch.zeros((slots, 4), dtype=torch.int64, device=dev)
    fit[live] = torch.stack([N, lam1, lam2, lam3], -1)
    counts = torch.stack([torch.tensor(M, device=dev), (N >= min_nb).sum(), given.sum(), torch.tensor(0, device=dev)])
    return normal, fit, counts, C.double()


def pose_error(pose, truth):
    r = pose[:9].reshape(3, 3) @ truth[:9].reshape(3, 3).T
    return [float(np.degrees(np.arccos(np.clip((np.trace(r) - 1) / 2, -1, 1)))), float(np.linalg.norm(pose[9:] - truth[9:]))]


def walled_cells(side):
    """The street with what a road has beside it: the ground plane, two walls along x, 30 cells to either side of the middle and 12 cells
    high, and hollow boxes of 10 x 6 x 7 cells - surfaces only, as a camera sees them - every 40 cells along x on both sides of the middle:
    the only evidence along the street.  int64 [V,3] cells, shuffled."""
    g = np.arange(side)
    ground = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3)
    walls = np.concatenate([np.stack(np.meshgrid(g, [side // 2 + dy], np.arange(1, 13), indexing="ij"), -1).reshape(-1, 3) for dy in (-30, 30)])
    box = np.stack(np.meshgrid(np.arange(10), np.arange(6), np.arange(1, 8), indexing="ij"), -1).reshape(-1, 3)
    box = box[(box[:, 0] % 9 == 0) | (box[:, 1] % 5 == 0) | (box[:, 2] == 7)]  # the four sides and the top
    corners = np.stack(np.meshgrid(np.arange(20, side - 20, 40), [side // 2 - 18, side // 2 + 12], [0], indexing="ij"), -1).reshape(-1, 1, 3)
    cells = np.concatenate([ground, walls, (corners + box).reshape(-1, 3)])
    return cells[np.random.default_rng(3).permutation(len(cells))]


def measure(a, cells, scene, time_normals):
    """One scene: the normals' times (time_normals), then the rounds and the loops of its two frames -> the scene's dict."""
    rigmod = importlib.import_module(PKG + ".rig")
    eng = importlib.import_module(PKG + ".engine")
    sv = importlib.import_module(PKG + ".stereo_vision.sv")
    L, A, Y = eng.voxel_map_lib(), eng.voxel_align_lib(), eng.voxel_normals_lib()
    size, side = a.size, a.side
    st = torch.cuda.current_stream().cuda_stream

    cap = 65536
    B = -(-len(cells) // cap)
    xyz = np.zeros((B * cap, 3), np.float32)
    xyz[:len(cells)] = (cells + 0.5) * size
    counts = np.full(B, cap, np.int32)
    counts[-1] = len(cells) - (B - 1) * cap
    m = rigmod.VoxelMap((0.0, 0.0, 0.0), (side * size, side * size, 16 * size), size, len(cells) + len(cells) // 8)
    m.update(torch.from_numpy(xyz.reshape(B, cap, 3)).cuda(), None, None, torch.from_numpy(counts).cuda(), np.tile(sv.voxel_map_pose(0.0, 0.0, 0.0), (B, 1)))
    assert m.stats()["claimed"] == len(cells) and not m.stats()["overflowed"]
    params, buf = m.params, m.buffer
    spec, nbytes = eng.voxel_map_spec(params), L.sv_voxel_map_bytes(params["capacity"])
    slots = int(L.sv_voxel_map_slots(params["capacity"]))
    table = buf[4:4 + 11 * slots].view(slots, 11)
    res = {"scene": scene, "size": size, "voxels_in_the_map": len(cells), "capacity": params["capacity"], "table_slots": slots, "reps": a.reps, "normals": [], "rounds": []}

    kept = None
    for mm in ((16, 32) if time_normals else ()):
        dirs = eng.voxel_normal_table(sv.voxel_normal_dirs(mm), buf.device)
        K = int(dirs.shape[0])
        out = eng.voxel_map_normals(buf, params, dirs, want_fit=True)

        def call(fit=False, prune=True, dirs=dirs, K=K, out=out):
            eng.debug_voxel_normals(0, True, prune)
            rc = Y.sv_voxel_normals_device(buf.data_ptr(), nbytes, ctypes.byref(spec), dirs.data_ptr(), K, 5, 64, 16, 1, 1, 0, out.normal.data_ptr(), slots,
                                           out.fit.data_ptr() if fit else None, out.counts.data_ptr(), st)
            assert rc == 0, L.sv_last_error(None)

        want_normal, want_fit, want_counts, C = torch_normals(params, table, dirs, 5, 64, 16)
        for fit, prune in ((True, True), (False, True), (False, False)):
            out.normal.fill_(-7)
            call(fit, prune)
            assert torch.equal(out.normal, want_normal) and torch.equal(out.counts, want_counts) and (not fit or torch.equal(out.fit, want_fit)), \
                "the kernel and the torch form disagree at m = %d (fit %s, pruning %s)" % (mm, fit, prune)
        try:
            t = street.time_beside({"normal": lambda: call(False, True), "normal_unpruned": lambda: call(False, False), "fit": lambda: call(True, True),
                                    "fit_unpruned": lambda: call(True, False)}, a.reps)
        finally:
            eng.debug_voxel_normals(0, True, True)
        cnt = [int(v) for v in want_counts.cpu()]
        entry = {"m": mm, "directions": K, "members": cnt[0], "enough_neighbours": cnt[1], "normals": cnt[2], "calls": t,
                 "directions_tried_per_us": {"normal": cnt[1] * K / t["normal"]["us"], "fit": cnt[0] * K / t["fit"]["us"]}}
        entry["torch_same_definition_us"] = street.time_events(lambda: torch_normals(params, table, dirs, 5, 64, 16), 3)
        some = C[:131072].contiguous()  # a batch of that many 3 x 3 matrices; the whole map is 7.6 times as many
        entry["torch_eigh_of_131072_us"] = street.time_events(lambda: torch.linalg.eigh(some), 3)
        entry["torch_over_kernel"] = entry["torch_same_definition_us"]["us"] / t["fit"]["us"]
        print("normals m = %d (%d directions): %d members, %d with enough neighbours, %d normals; %.0f us (unpruned %.0f), with fit %.0f us (unpruned %.0f); %.0f and %.0f "
              "directions / us; torch, the same definition: %.0f us (%.1fx of the call with fit); torch.linalg.eigh of 131072 of the covariances: %.0f us"
              % (mm, K, *cnt[:3], t["normal"]["us"], t["normal_unpruned"]["us"], t["fit"]["us"], t["fit_unpruned"]["us"], entry["directions_tried_per_us"]["normal"],
                 entry["directions_tried_per_us"]["fit"], entry["torch_same_definition_us"]["us"], entry["torch_over_kernel"], entry["torch_eigh_of_131072_us"]["us"]), flush=True)
        res["normals"].append(entry)
        if mm == 16:
            kept = eng.voxel_map_normals(buf, params, dirs)

    if kept is None:
        kept = eng.voxel_map_normals(buf, params, sv.voxel_normal_dirs())
        print("%s: %s voxels, members / enough neighbours / normals %s" % (scene, len(cells), kept.counts.cpu().numpy()[:3].tolist()), flush=True)
    res["normals_of_the_loops"] = [int(v) for v in kept.counts.cpu().numpy()[:3]]
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.sv_voxel_align_device.restype, parent.sv_voxel_align_device.argtypes = eng.STAGE_SIGNATURES["voxel_align"]["sv_voxel_align_device"]
    truth = sv.voxel_map_pose(0.5 * side * size + 0.07, 0.5 * side * size - 0.04, 0.3, 1.2)
    cr, sr, cp, sp, cy, sy = np.cos(0.003), np.sin(0.003), np.cos(-0.004), np.sin(-0.004), np.cos(0.006), np.sin(0.006)
    off = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]]) @ np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    start = np.concatenate([(off @ truth[:9].reshape(3, 3)).reshape(9), truth[9:] + np.array([0.5, -0.4, 0.3]) * size])[None]
    origin = sv.voxel_align_origin(params, start)
    max_d2 = sv.voxel_align_max_d2(1.0)
    for name, frame in street.frames_of(cells, size, side, 20.0, a.cloud_rows, truth).items():
        fx, fc = torch.from_numpy(frame).cuda(), torch.tensor([frame.shape[1]], dtype=torch.int32, device="cuda")
        rows = frame.shape[1]
        pose_t, origin_t = torch.from_numpy(start).cuda(), torch.from_numpy(origin).cuda()
        point = eng.voxel_map_align_sums(buf, params, fx, None, fc, pose_t, origin_t)
        plane = eng.voxel_map_align_plane_sums(buf, params, fx, None, fc, pose_t, origin_t, kept)
        need, need_plane = ctypes.c_size_t(), ctypes.c_size_t()
        assert A.sv_voxel_align_workspace(rows, 1, ctypes.byref(need)) == 0 and Y.sv_voxel_plane_align_workspace(rows, 1, ctypes.byref(need_plane)) == 0
        ws = torch.empty((need_plane.value // 8,), dtype=torch.int64, device="cuda")
        sums_parent = torch.zeros_like(point.sums)

        def point_round(lib=A, sums=point.sums):
            rc = lib.sv_voxel_align_device(buf.data_ptr(), nbytes, ctypes.byref(spec), fx.data_ptr(), 0, None, fc.data_ptr(), pose_t.data_ptr(), origin_t.data_ptr(), 1, rows, max_d2,
                                           1, 1, 0, sums.data_ptr(), None, None, ws.data_ptr(), need.value, st)
            assert rc == 0

        def plane_round():
            rc = Y.sv_voxel_plane_align_device(buf.data_ptr(), nbytes, ctypes.byref(spec), fx.data_ptr(), 0, None, fc.data_ptr(), pose_t.data_ptr(), origin_t.data_ptr(), 1, rows,
                                               max_d2, 1, 1, 0, kept.normal.data_ptr(), slots, kept.dirs.data_ptr(), int(kept.dirs.shape[0]), plane.sums.data_ptr(), None, None, None,
                                               ws.data_ptr(), need_plane.value, st)
            assert rc == 0, L.sv_last_error(None)

        fns = {"point": point_round, "plane": plane_round}
        if parent is not None:
            fns["point_parent"] = lambda: point_round(parent, sums_parent)
        t = street.time_beside(fns, a.reps)
        if parent is not None:
            assert torch.equal(sums_parent, point.sums), "the parent's point round gives other sums"
        entry = {"run": name, "rows": rows, "inside": int(plane.sums[0, 0]), "pairs": int(plane.sums[0, 1]), "planes": int(plane.sums[0, 2]), "one_round_us": t,
                 "plane_over_point": t["plane"]["us"] / t["point"]["us"]}
        loops = {}
        for method, kw in (("point", {}), ("plane", {}), ("plane_normals_kept", dict(normals=kept))):
            run = lambda: eng.voxel_map_align(buf, params, fx, None, fc, start, iterations=30, method=method.split("_")[0], **kw)  # noqa: E731
            got = run()
            loops[method] = {"rounds": int(got.rounds), "start_error": pose_error(start[0], truth), "end_error": pose_error(got.poses[0], truth),
                             "pairs_per_round": got.pairs[:, 0].tolist(), "wall_us": street.time_host(run, max(a.reps // 3, 3))}

        def both():  # the planes first, then the means from where the planes ended
            first = eng.voxel_map_align(buf, params, fx, None, fc, start, iterations=30, method="plane", normals=kept)
            return first, eng.voxel_map_align(buf, params, fx, None, fc, first.poses, iterations=30)

        first, then = both()
        loops["plane_then_point"] = {"rounds": [int(first.rounds), int(then.rounds)], "end_error": pose_error(then.poses[0], truth), "wall_us": street.time_host(both, max(a.reps // 3, 3))}
        entry["loops_to_convergence"] = loops
        print("%s, %s: %d rows, %d pairs, %d plane pairs; one round: point %.1f us%s, plane %.1f us (%.2fx); to convergence: point %d rounds, %.0f us, %.4f deg %.4f m; plane %d rounds, "
              "%.0f us (%.0f us with the normals kept), %.4f deg %.4f m; plane, then point from there: %d + %d rounds, %.0f us, %.4f deg %.4f m"
              % (scene, name, rows, entry["pairs"], entry["planes"], t["point"]["us"], " (the parent's build %.1f us)" % t["point_parent"]["us"] if parent is not None else "", t["plane"]["us"],
                 entry["plane_over_point"], loops["point"]["rounds"], loops["point"]["wall_us"]["us"], *loops["point"]["end_error"], loops["plane"]["rounds"], loops["plane"]["wall_us"]["us"],
                 loops["plane_normals_kept"]["wall_us"]["us"], *loops["plane"]["end_error"], *loops["plane_then_point"]["rounds"], loops["plane_then_point"]["wall_us"]["us"],
                 *loops["plane_then_point"]["end_error"]), flush=True)
        res["rounds"].append(entry)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--size", type=float, default=0.2)
    ap.add_argument("--side", type=int, default=800, help="cells of the ground plane per axis")
    ap.add_argument("--cloud-rows", type=int, default=300000)
    ap.add_argument("--parent-lib", default="", help="libstereo_vision_hip.so of the parent commit, for its point round beside this build's")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = {"scenes": [measure(a, street.street_cells(a.side), "street", True), measure(a, walled_cells(a.side), "walled_street", False)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
