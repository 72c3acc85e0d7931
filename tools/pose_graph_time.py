#!/usr/bin/env python3
"""The pose graph of group (AE) on synthetic drives (HIP events, medians of --reps calls after warm-up, min / max beside the median; one
process, every buffer allocated before anything is timed).  A drive is a winding chain of N poses with N / 100 loop edges between random
frames, measurements 10 mrad and 5 cm off the truth, the start 30 mrad and 0.3 m off.
  linearise    sv_pose_graph_linearize_device, two kernels;
  iteration    sv_pose_graph_pcg_device with 16 iterations minus the same call with none, over 16 - three kernels an iteration -, and
               the same 16 iterations once `done` is set, where every kernel returns at its first instruction: the launch floor;
  to_tol       iterations and wall time to tol = 1e-8 on a pure chain with one loop from the last frame to the first, where block-Jacobi
               has to carry the loop's error along the whole chain;
  optimize     engine.pose_graph_optimize, by the host's clock, split into the device's part of a round (upload, linearise, solve, the
               waits, the read-back) and the host's (pose_exp and the product per pose, the gate);
beside the same definition in torch ops on the same device (gathers, index_add_, bmm with the inverted blocks), per iteration, and the
dense numpy solve of the same linear system at N = 1 000 by the host's clock.  Before anything is timed the torch form's and the dense
solve's x must agree with the kernels' to a relative 1e-6.  Nothing is asserted about speed.

    timeout -k 10 900 python tools/pose_graph_time.py [--reps 21] [--out profiles/pose_graph_time.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_align_time as street  # noqa: E402 (the timers)

PKG = street.PKG
LAM, TOL = 1e-6, 1e-8


def rot(om):
    angle = np.sqrt((om * om).sum(1))
    K = np.zeros((len(om), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -om[:, 2], om[:, 1], om[:, 2], -om[:, 0], -om[:, 1], om[:, 0]
    a = np.where(angle < 1e-8, 1.0, angle)
    s, c = np.where(angle < 1e-8, 1.0, np.sin(a) / a), np.where(angle < 1e-8, 0.5, (1.0 - np.cos(a)) / (a * a))
    return np.eye(3)[None] + s[:, None, None] * K + c[:, None, None] * (K @ K)


def pack(R, t):
    return np.ascontiguousarray(np.concatenate([R.reshape(-1, 9), t.reshape(-1, 3)], 1))


def nudged(P, rng, s_rot, s_trans):
    R, t = P[:, :9].reshape(-1, 3, 3), P[:, 9:]
    return pack(R @ rot(rng.normal(0.0, s_rot, (len(P), 3))), t + (R @ rng.normal(0.0, s_trans, (len(P), 3, 1)))[:, :, 0])


def drive(N, loops, seed):
    """-> poses, fixed, i, j, Z, w of a chain of N poses with the loop edges `loops` [(i, j), ...]."""
    rng = np.random.default_rng(seed)
    k = np.arange(N, dtype=np.float64)
    truth = pack(rot(np.stack([0.1 * np.sin(k / 50.0), 0.1 * np.cos(k / 70.0), 0.02 * k], 1)), np.cumsum(rng.normal(0.0, 0.6, (N, 3)) + [0.8, 0.0, 0.0], 0))
    i = np.concatenate([np.arange(N - 1), [p[0] for p in loops]]).astype(np.int32)
    j = np.concatenate([np.arange(1, N), [p[1] for p in loops]]).astype(np.int32)
    Ra, ta, Rb, tb = truth[i, :9].reshape(-1, 3, 3), truth[i, 9:], truth[j, :9].reshape(-1, 3, 3), truth[j, 9:]
    Rt = Ra.transpose(0, 2, 1)
    Z = nudged(pack(Rt @ Rb, (Rt @ (tb - ta)[:, :, None])[:, :, 0]), rng, 0.01, 0.05)
    w = np.ascontiguousarray(10.0 ** rng.uniform(0.0, 2.0, (len(i), 2)))
    fixed = np.zeros(N, bool)
    fixed[0] = True
    poses = nudged(truth, rng, 0.03, 0.3)
    poses[0] = truth[0]
    return poses, fixed, i, j, Z, w


def random_loops(N, seed):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, N, (max(N // 100, 1), 2))
    return [tuple(r) for r in p[p[:, 0] != p[:, 1]].tolist()]


def torch_form(fixed, i, j, w, lin, lam):
    """The same PCG in torch ops -> (start, iterate): closures over the state, one iteration a call; x is state["x"]."""
    dev = lin["b"].device
    N = lin["b"].shape[0]
    i, j = i.long(), j.long()
    M = lin["M"]
    R, t = M[:, :9].reshape(-1, 3, 3), M[:, 9:]
    T = torch.zeros_like(R)
    T[:, 0, 1], T[:, 0, 2], T[:, 1, 0], T[:, 1, 2], T[:, 2, 0], T[:, 2, 1] = -t[:, 2], t[:, 1], t[:, 2], -t[:, 0], -t[:, 1], t[:, 0]
    Ad = torch.zeros((len(i), 6, 6), dtype=torch.float64, device=dev)
    Ad[:, :3, :3], Ad[:, 3:, 3:], Ad[:, 3:, :3] = R, R, T @ R
    w6 = torch.repeat_interleave(w, 3, dim=1)
    free = (~fixed.bool()).double()[:, None]
    # the diagonal blocks, inverted once
    B = torch.zeros((N, 6, 6), dtype=torch.float64, device=dev)
    B.index_add_(0, j, torch.diag_embed(w6))
    B.index_add_(0, i, Ad.transpose(1, 2) @ (w6[:, :, None] * Ad))
    Binv = torch.from_numpy(np.linalg.inv((B + lam * torch.eye(6, dtype=torch.float64, device=dev)).cpu().numpy())).to(dev)  # on the host: once, not timed
    s = {}

    def H(x):
        g = w6 * (x[j] - (Ad @ x[i][:, :, None])[:, :, 0])
        q = torch.zeros_like(x)
        q.index_add_(0, j, g)
        q.index_add_(0, i, -(Ad.transpose(1, 2) @ g[:, :, None])[:, :, 0])
        return (q + lam * x) * free

    def start():
        s["x"], s["r"] = torch.zeros_like(lin["b"]), lin["b"].clone()
        s["z"] = (Binv @ s["r"][:, :, None])[:, :, 0]
        s["p"], s["rz"] = s["z"].clone(), (s["r"] * s["z"]).sum()

    def iterate():
        q = H(s["p"])
        alpha = s["rz"] / (s["p"] * q).sum()
        s["x"] = s["x"] + alpha * s["p"]
        s["r"] = s["r"] - alpha * q
        s["z"] = (Binv @ s["r"][:, :, None])[:, :, 0]
        rz = (s["r"] * s["z"]).sum()
        s["p"] = s["z"] + (rz / s["rz"]) * s["p"]
        s["rz"] = rz

    return start, iterate, s, H


def dense_solve(fixed, i, j, w, M, b, lam):
    """H assembled densely on the host from the linearisation's M, and np.linalg.solve."""
    N = len(b)
    H = np.zeros((6 * N, 6 * N))
    for e in range(len(i)):
        R, t = M[e, :9].reshape(3, 3), M[e, 9:]
        Tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
        J = {int(i[e]): -np.block([[R, np.zeros((3, 3))], [Tx @ R, R]]), int(j[e]): np.eye(6)}
        W = np.diag(np.repeat(w[e], 3))
        for a_, Ja in J.items():
            for c_, Jc in J.items():
                H[6 * a_:6 * a_ + 6, 6 * c_:6 * c_ + 6] += Ja.T @ W @ Jc
    H += lam * np.eye(6 * N)
    free = np.repeat(~fixed, 6)
    x = np.zeros(6 * N)
    x[free] = np.linalg.solve(H[np.ix_(free, free)], b.reshape(-1)[free])
    return x.reshape(N, 6)


def save(res, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    eng = importlib.import_module(PKG + ".engine")
    sv = importlib.import_module(PKG + ".stereo_vision.sv")
    L = eng.pose_graph_lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    res = {"reps": a.reps, "lam": LAM, "tol": TOL, "launches": {"per_iteration": 3, "per_call_of_the_entry": 1, "start_of_a_solve": 2, "linearise": 2}, "sizes": {}}

    for N in [int(v) for v in a.sizes.split(",")]:
        poses, fixed, i, j, Z, w = drive(N, random_loops(N, N), N + 1)
        E = len(i)
        words = sv.pose_graph_words(N, i, j)
        fixed_d, i_d, j_d, w_d, row_start, inc = up(fixed.astype(np.uint8)), up(i), up(j), up(w), up(words[0]), up(words[1])
        P_d, Z_d = up(poses), up(Z)
        lin = eng.pose_graph_linearize(P_d, fixed_d, i_d, j_d, Z_d, w_d, LAM, (row_start, inc))
        x = torch.zeros((N, 6), dtype=torch.float64, device=dev)
        need = ctypes.c_size_t()
        assert L.sv_pose_graph_workspace(N, E, ctypes.byref(need)) == 0
        ws = torch.zeros(need.value, dtype=torch.uint8, device=dev)

        def pcg(iters, tol, spec_of={}):
            spec = spec_of.setdefault(tol, eng.SvPoseGraphSpec(LAM, tol))
            assert L.sv_pose_graph_pcg_device(fixed_d.data_ptr(), N, i_d.data_ptr(), j_d.data_ptr(), w_d.data_ptr(), E, row_start.data_ptr(), inc.data_ptr(), lin["M"].data_ptr(),
                                              lin["b"].data_ptr(), lin["factor"].data_ptr(), ctypes.byref(spec), 0, iters, x.data_ptr(), ws.data_ptr(), need.value, st) == 0

        # the torch form agrees with the kernels after the same 32 iterations
        x_dev, state = eng.pose_graph_solve(fixed_d, i_d, j_d, w_d, lin, LAM, max_iters=32, tol=0.0)
        start, iterate, s, H = torch_form(fixed_d, i_d, j_d, w_d, lin, LAM)
        start()
        for _ in range(32):
            iterate()
        gap = float((s["x"] - x_dev).abs().max()) / float(x_dev.abs().max())
        assert state["iteration"] == 32 and gap <= 1e-6, (N, state, gap)
        # to tol, by the host's clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x_dev, state = eng.pose_graph_solve(fixed_d, i_d, j_d, w_d, lin, LAM, max_iters=min(40 * N, 400000), tol=TOL, round=1024)
        to_tol_s = time.perf_counter() - t0
        model = lambda v: float(0.5 * (v * H(v)).sum() - (v * lin["b"]).sum())  # noqa: E731 (the quadratic the solve minimises)

        fns = {"linearise": lambda: eng.pose_graph_linearize(P_d, fixed_d, i_d, j_d, Z_d, w_d, LAM, (row_start, inc), lin),
               "start_and_finish": lambda: pcg(0, 0.0), "sixteen": lambda: pcg(16, 0.0), "sixteen_done": lambda: pcg(16, 1.0)}
        t = street.time_beside(fns, a.reps)
        start()
        torch_t = street.time_events(iterate, a.reps)
        per = (t["sixteen"]["us"] - t["start_and_finish"]["us"]) / 16.0
        floor = (t["sixteen_done"]["us"] - t["start_and_finish"]["us"]) / 16.0
        row = {"edges": E, "loop_edges": E - (N - 1), "workspace_bytes": need.value, "timed_us": t, "iteration_us": per, "iteration_us_once_done": floor,
               "torch_form_iteration_us": torch_t, "torch_form_over_kernels": torch_t["us"] / per, "torch_form_gap_after_32_iterations": gap,
               "to_tol": dict(state, wall_s=to_tol_s)}
        print("N = %7d: linearise %.1f us, an iteration %.2f us (%.2f us once done), torch form %.1f us (%.1fx); to tol %s in %.3f s" % (
            N, t["linearise"]["us"], per, floor, torch_t["us"], torch_t["us"] / per, state, to_tol_s), flush=True)

        if N <= 1000:  # the dense numpy solve of the same system
            M_h, b_h = lin["M"].cpu().numpy(), lin["b"].cpu().numpy()
            t0 = time.perf_counter()
            x_dense = dense_solve(fixed, i, j, w, M_h, b_h, LAM)
            dense_s = time.perf_counter() - t0
            q_dense, q_pcg = model(up(x_dense)), model(x_dev)
            gap = abs(q_pcg - q_dense) / abs(q_dense)
            assert state["done"] and gap <= 1e-6, (state, q_dense, q_pcg)  # the dense check's bound, on the quadratic both minimise
            row["dense_numpy"] = {"assemble_and_solve_s": dense_s, "model_cost_dense": q_dense, "model_cost_pcg": q_pcg, "relative_gap": gap}
            print("            dense numpy %.2f s, the kernels to tol %.4f s, relative gap of the model cost %.2g" % (dense_s, to_tol_s, gap), flush=True)
        res["sizes"][str(N)] = row
        save(res, a.out)

    # a pure chain with one loop: what block-Jacobi costs
    res["chain_with_one_loop"] = {}
    for N in (1000, 10000):
        poses, fixed, i, j, Z, w = drive(N, [(N - 1, 0)], 7)
        lin = eng.pose_graph_linearize(up(poses), fixed, i, j, Z, w, LAM)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, state = eng.pose_graph_solve(fixed, i, j, w, lin, LAM, max_iters=40 * N, tol=TOL, round=1024)
        wall = time.perf_counter() - t0
        res["chain_with_one_loop"][str(N)] = dict(state, wall_s=wall, us_per_iteration=1e6 * wall / max(state["iteration"], 1))
        save(res, a.out)
        print("chain of %d with one loop: %s in %.3f s" % (N, state, wall), flush=True)

    # a whole optimize, by the host's clock
    N = 1000
    poses, fixed, i, j, Z, w = drive(N, random_loops(N, N), N + 1)
    g = sv.pose_graph(poses, [(i, j, Z, w, (np.arange(len(i)) >= N - 1).astype(np.int32))], fixed)
    eng.pose_graph_optimize(g, rounds=1, device=dev)  # warm-up
    inside = [0.0]

    def timed(step):
        def run(*args):
            t0 = time.perf_counter()
            out = step(*args)
            inside[0] += time.perf_counter() - t0
            return out
        return run

    t0 = time.perf_counter()
    _, stats = eng.pose_graph_optimize(g, rounds=10, device=dev, wrap_step=timed)
    total = time.perf_counter() - t0
    res["optimize"] = {"poses": N, "edges": len(i), "rounds": stats["rounds"], "iterations": stats["iterations"], "converged": stats["converged"], "total_s": total, "device_part_s": inside[0],
                       "host_part_s": total - inside[0], "costs": stats["costs"] + [stats["cost"]]}
    print("optimize, N = %d: %d rounds, %s iterations, %.3f s: %.3f s in the rounds' device part (waits included), %.3f s on the host" % (
        N, stats["rounds"], stats["iterations"], total, inside[0], total - inside[0]), flush=True)
    res["not_measured"] = ["counters (rocprofv3 --pmc)", "a chain of 100 000 with one loop to tol", "a preconditioner beyond block-Jacobi", "graphs of more than one device"]
    save(res, a.out)


if __name__ == "__main__":
    main()
