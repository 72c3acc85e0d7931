#!/usr/bin/env python3
"""Stereo visual odometry on the committed KITTI frames 0 .. 3 at full size (HIP events, median of --reps calls after warm-up, min / max
beside the median; one process).  The frames are rectified already, so the rig is two equal pinhole cameras (f 721.54, b 0.537 m).
  (a) us per call of sv_flow_match_device for kitti0 -> 1 at step 8, r 4, into pre-allocated outputs and workspace: the cold-start window
      (+-64 x +-24 from the identity) and +-8 x +-8 under a guess of 1.16 m forward; per call the lattice points that carry a disparity
      times the window's candidates per microsecond, and the bytes their sums of absolute differences read per second (81 a candidate) -
      candidates whose patch would leave the image are counted, so both are upper bounds by the share of such candidates;
  (b) us per call of sv_flow_pose_sums_device for the matches of (a)'s guessed window;
  (c) StereoRig.odometry of the four frames per frame beside StereoRig.disparity alone, by the host's clock around a synchronise;
  (d) the unfused form of the +-8 window on the same device with torch ops: the (2 r + 1)^2 patches of cur unfolded once per call, the
      candidates' patches gathered per point, |a - b| summed, the best by min() and the second by a masked min().  Before anything is
      timed both forms must agree on every point's best cost.
The yardstick is never the code under test.  Nothing is asserted about speed.

    timeout -k 10 600 python tools/flow_time.py [--reps 21] [--out profiles/flow_time.json]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd"
MATRIX = "%s: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: d\n   data: [ %s ]\n"
K = "721.54, 0.0, 609.56, 0.0, 721.54, 172.85, 0.0, 0.0, 1.0"
YML = ("%YAML:1.0\n" + MATRIX % ("K1", 3, 3, K) + MATRIX % ("K2", 3, 3, K) + MATRIX % ("D1", 1, 5, "0.0, 0.0, 0.0, 0.0, 0.0") + MATRIX % ("D2", 1, 5, "0.0, 0.0, 0.0, 0.0, 0.0")
       + MATRIX % ("R", 3, 3, "1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0") + "T: [ -0.537, 0.0, 0.0 ]\n")
GUESS = np.array([[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, -1.16]])


def events(fn, reps, warm=3):
    """{"median_us", "min_us", "max_us"} of `reps` calls of fn, each between two HIP events, after `warm` calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0)
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out))}


def host_clock(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out))}


def torch_match(prev, cur, pts, centres, r, wx, wy):
    """Best and second cost per point, with torch ops: pts and centres int64 [P,2] = (u, v); every candidate's patch lies inside the image
    (the caller keeps the points whose windows do).  -> (best int32 [P], index int64 [P], second int32 [P])."""
    side = 2 * r + 1
    H, W = cur.shape
    table = torch.nn.functional.unfold(cur[None, None].float(), (side, side))[0].t().to(torch.int16)  # [(H - 2r) (W - 2r), side^2]
    ptab = torch.nn.functional.unfold(prev[None, None].float(), (side, side))[0].t().to(torch.int16)
    cols = W - 2 * r
    dy, dx = torch.meshgrid(torch.arange(-wy, wy + 1, device=cur.device), torch.arange(-wx, wx + 1, device=cur.device), indexing="ij")
    dx, dy = dx.reshape(-1), dy.reshape(-1)
    at = (centres[:, 1:2] + dy[None] - r) * cols + (centres[:, 0:1] + dx[None] - r)  # [P,C]
    mine = ptab[(pts[:, 1] - r) * cols + (pts[:, 0] - r)]  # [P,side^2]
    best = torch.empty(len(pts), dtype=torch.int32, device=cur.device)
    index = torch.empty(len(pts), dtype=torch.int64, device=cur.device)
    second = torch.empty(len(pts), dtype=torch.int32, device=cur.device)
    for lo in range(0, len(pts), 1024):  # a gather of 1024 x C x side^2 at a time
        hi = min(lo + 1024, len(pts))
        cost = (table[at[lo:hi]] - mine[lo:hi, None]).abs().sum(-1, dtype=torch.int32)  # [p,C]
        b, i = cost.min(1)
        near = ((dx[None] - dx[i][:, None]).abs() <= 1) & ((dy[None] - dy[i][:, None]).abs() <= 1)
        best[lo:hi], index[lo:hi], second[lo:hi] = b, i, cost.masked_fill(near, 2 ** 30).min(1)[0]
    return best, index, second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_time needs the GPU: nothing is measured without one")
    eng, rigmod, sv = (importlib.import_module(PKG + "." + m) for m in ("engine", "rig", "stereo_vision.sv"))
    golden = os.path.join(ROOT, "tests", "golden")
    ls = np.stack([np.repeat(np.asarray(Image.open(os.path.join(golden, "kitti%d_left.png" % k)))[..., None], 3, -1) for k in range(4)])
    rs = np.stack([np.repeat(np.asarray(Image.open(os.path.join(golden, "kitti%d_right.png" % k)))[..., None], 3, -1) for k in range(4)])
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "rectified.yml"), "w") as f:
            f.write(YML)
        rig = rigmod.StereoRig(1242, 375, calibration=os.path.join(tmp, "rectified.yml"), params=eng.SvParams.driver(127))
    left, right = torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "frames": "kitti0..3, 1242 x 375, disp_max 127", "step": 8, "r": 4}
    try:
        gl, gr = rig.frontend(left, right)
        d1, _ = rig.engine.process_device(gl, gr, want_d2=False)
        camera = rig.render_camera(1.0)
        prev, cur, dp, dc = gl[0:1], gl[1:2], d1[0:1], d1[1:2]
        r, step = 4, 8
        dq = sv._flow_dq(dp[0].cpu().numpy())
        v, u = np.meshgrid(np.arange(0, 375, step), np.arange(0, 1242, step), indexing="ij")
        ok = (dq[v, u] > 0) & (u >= r) & (u < 1242 - r) & (v >= r) & (v < 375 - r)
        res["points"] = int(ok.sum())
        for name, (wx, wy), guess in (("cold_64x24", (64, 24), None), ("guess_8x8", (8, 8), GUESS)):
            out = eng.flow_match(prev, cur, dp, dc, camera, guess, step=step, r=r, wx=wx, wy=wy, capacity=8192)
            ws = torch.empty((1242 // step + 1) * (375 // step + 1) * 8, dtype=torch.int32, device="cuda")
            t = events(lambda: eng.flow_match(prev, cur, dp, dc, camera, guess, step=step, r=r, wx=wx, wy=wy, capacity=8192, out=out, workspace=ws), args.reps)
            cands = res["points"] * (2 * wx + 1) * (2 * wy + 1)
            res[name] = dict(t, matches=int(out.counts[0]), candidates=cands, candidates_per_us=cands / t["median_us"], sad_bytes_per_s=cands * 81 / (t["median_us"] * 1e-6))
        # (b) one round of sums on the guessed window's matches
        poses = torch.from_numpy(GUESS).cuda()
        sums = torch.empty((1, 32), dtype=torch.int64, device="cuda")
        res["sums_round"] = dict(events(lambda: eng.flow_pose_sums(out.matches, out.counts, camera, poses, 48, 32, out=sums), args.reps), matches=int(out.counts[0]))
        # (c) the whole odometry per frame beside the disparity alone
        odo = host_clock(lambda: rig.odometry(left, right), max(args.reps // 3, 3))
        dis = host_clock(lambda: rig.disparity(left, right), max(args.reps // 3, 3))
        got = rig.odometry(left, right)
        res["odometry_per_frame"] = {k: x / 4.0 for k, x in odo.items()}
        res["disparity_per_frame"] = {k: x / 4.0 for k, x in dis.items()}
        res["rel_t"] = got["rel"][:, 9:].tolist()
        res["inliers"] = got["inliers"].tolist()
        # (d) torch on the same device, +-8 around the guess; the points whose whole window lies inside the image
        m = eng.flow_match(prev, cur, dp, dc, camera, GUESS, step=step, r=r, wx=8, wy=8, ratio=256, max_cost=2 ** 30, capacity=8192)
        rows = m.matches[0, :int(m.counts[0])].long()
        costs = m.cost[0, :int(m.counts[0])]
        keep = (rows[:, 3] >= r + 8) & (rows[:, 3] < 1242 - r - 8) & (rows[:, 4] >= r + 8) & (rows[:, 4] < 375 - r - 8)
        x, y, z = sv._flow_move(GUESS[0], *sv._flow_point(sv.flow_camera(camera), rows[:, 0].cpu().numpy(), rows[:, 1].cpu().numpy(), rows[:, 2].cpu().numpy()))
        cam = sv.flow_camera(camera)
        cx, cy = np.floor(((cam["f"] * x) / z + cam["cx"]) + 0.5).astype(np.int64), np.floor(((cam["f"] * y) / z + cam["cy"]) + 0.5).astype(np.int64)
        centres = torch.from_numpy(np.stack([cx, cy], 1)).cuda()
        keep &= (centres[:, 0] >= r + 8) & (centres[:, 0] < 1242 - r - 8) & (centres[:, 1] >= r + 8) & (centres[:, 1] < 375 - r - 8)
        pts, centres, costs = rows[keep][:, :2], centres[keep], costs[keep]
        b, _, s = torch_match(prev[0], cur[0], pts, centres, r, 8, 8)
        if not (torch.equal(b, costs[:, 0]) and torch.equal(s, costs[:, 1])):
            raise SystemExit("the torch form and the kernel disagree on a best or second cost")
        t = events(lambda: torch_match(prev[0], cur[0], pts, centres, r, 8, 8), max(args.reps // 3, 3))
        res["torch_8x8"] = dict(t, points=int(len(pts)), note="the matched points only: fewer than the kernel's, no disparity test, no ratio test, no compaction")
        res["fused_is_faster"] = bool(res["guess_8x8"]["median_us"] < t["median_us"])
    finally:
        rig.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
