"""In-tree build of libstereo_vision_hip.so (hipcc, gfx950 only).

    python build.py            # incremental
    python build.py --force

Flags that matter for parity: -ffp-contract=off (the reference's serial path has no FMA) and
correctly rounded fp32 divide (plane/edge-line arithmetic of elas.cpp:894-906 must match x86 IEEE results).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libstereo_vision_hip.so")
SOURCES = ["kernels.hip", "delaunay_gpu.hip", "legacy_kernels.hip", "rig_kernels.hip", "top_view_kernels.hip", "box_kernels.hip", "cloud_kernels.hip", "ground_kernels.hip", "stixel_kernels.hip", "voxel_kernels.hip", "occupancy_kernels.hip", "occupancy_map_kernels.hip", "map_match_kernels.hip", "clearance_kernels.hip", "cost_kernels.hip", "frontier_kernels.hip", "view_kernels.hip", "voxel_map_kernels.hip", "voxel_match_kernels.hip", "voxel_carry_kernels.hip", "voxel_carve_kernels.hip", "voxel_render_kernels.hip", "voxel_flatten_kernels.hip", "voxel_cluster_kernels.hip", "voxel_align_kernels.hip", "voxel_normal_kernels.hip", "flow_kernels.hip", "warp_kernels.hip", "track_kernels.hip", "place_kernels.hip", "voxel_repose_kernels.hip", "pose_graph_kernels.hip", "engine.cpp", "host_stage.cpp", "legacy.cpp", "calib.cpp", "rig.cpp", "top_view.cpp", "box_positions.cpp",
           "cloud.cpp", "ground.cpp", "stixels.cpp", "voxel.cpp", "occupancy.cpp", "occupancy_map.cpp", "map_match.cpp", "clearance.cpp", "cost.cpp", "frontier.cpp", "view.cpp", "voxel_map.cpp", "voxel_match.cpp", "voxel_carry.cpp", "voxel_carve.cpp", "voxel_render.cpp", "voxel_flatten.cpp", "voxel_cluster.cpp", "voxel_align.cpp", "voxel_normals.cpp", "flow.cpp", "warp.cpp", "track.cpp", "place.cpp", "voxel_repose.cpp", "pose_graph.cpp", "dma_lanes.cpp"]
HEADERS = ["sv_kernels.h", "host_stage.h", "calib.h", "rig_kernels.h", "reproject.h", "top_view_kernels.h", "box_kernels.h", "cloud_kernels.h", "ground_kernels.h", "stixel_kernels.h", "voxel_kernels.h", "occupancy_kernels.h", "occupancy_map_kernels.h", "occupancy_map_cells.h", "map_match_kernels.h", "clearance_kernels.h", "cost_kernels.h", "frontier_kernels.h", "view_kernels.h", "voxel_map_kernels.h", "voxel_map_table.h", "voxel_match_kernels.h", "voxel_carry_kernels.h", "voxel_carve_kernels.h", "voxel_render_kernels.h", "voxel_flatten_kernels.h", "voxel_cluster_kernels.h", "voxel_align_kernels.h", "voxel_normal_kernels.h", "flow_kernels.h", "flow_point.h", "warp_kernels.h", "track_kernels.h", "place_kernels.h", "voxel_repose_kernels.h", "pose_graph_kernels.h", "stage_glue.h", "dma_lanes.h", "wave_ops.h", os.path.join("..", "..", "include", "stereo_vision_hip.h")]
COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unused-value"]
HOST = ["-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
DEVICE = ["--offload-arch=gfx950", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-rdc"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    hipcc = _hipcc()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    objs = []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        obj = os.path.join(objdir, src + ".o")
        objs.append(obj)
        if force or _stale(obj, [path] + hdrs):
            cmd = [hipcc] + COMMON + (DEVICE if src.endswith(".hip") else HOST) + ["-c", path, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    if force or _stale(LIB, objs):
        cmd = [hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB] + objs + ["-lpthread", "-ldl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
