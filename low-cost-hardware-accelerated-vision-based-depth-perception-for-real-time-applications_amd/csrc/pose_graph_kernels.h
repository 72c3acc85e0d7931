// Launch interface of pose_graph_kernels.hip (the pose graph of confirmed loops: one linearisation, and preconditioned conjugate
// gradients on it: pose_graph.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

enum {
    PG_THREADS = 256,     // a workgroup of every kernel: four wavefronts, a lane per pose or edge; a workgroup of poses is a chunk of a dot
    PG_STATE_BYTES = 64,  // the state words in front of the workspace
    PG_BLOCK_WORDS = 21,  // a symmetric 6 x 6 block: row p, column q <= p at p (p + 1) / 2 + q
    PG_LAUNCHES_PER_ITERATION = 3
};

// The state words of the solver, device memory.  `done` is read by the edge and the update kernel and written by the pose kernel,
// `done_seen` is read by the pose kernel and written by the update kernel: no kernel reads a word that one of its own workgroups writes.
struct PoseGraphState {
    int32_t iteration;  // iterations made
    int32_t done;       // rr <= tol^2 rr0 was seen
    double rr, rr0;
    int32_t done_seen;
    int32_t reserved[9];
};
static_assert(sizeof(PoseGraphState) == PG_STATE_BYTES, "the state is 64 bytes");

struct PoseGraphLinArgs {
    const double *poses;       // [n_poses][12]
    const uint8_t *fixed;      // [n_poses]
    const int32_t *ei, *ej;    // [n_edges]
    const double *Z;           // [n_edges][12]
    const double *w;           // [n_edges][2]
    const int32_t *row_start;  // [n_poses + 1]
    const int32_t *inc;        // [2 n_edges]
    double *M, *Wr, *chi2;     // [n_edges][12], [n_edges][6], [n_edges]
    double *b, *factor;        // [n_poses][6], [n_poses][21]
    double lam;
    int n_poses, n_edges;
};

struct PoseGraphPcgArgs {
    const uint8_t *fixed;
    const int32_t *ei, *ej;
    const double *w;
    const int32_t *row_start, *inc;
    const double *M, *b, *factor;
    double lam, tol2;
    double *x;                 // [n_poses][6]: the result
    double *r, *z, *p, *q;     // [n_poses][6] each, workspace
    double *g;                 // [n_edges][6], workspace
    double *prr[2], *prz[2];   // [chunks] each: the chunks' partials of <r, r> and <r, z>, by the parity of the iteration that reads them
    double *ppq;               // [chunks]: of <p, q>
    PoseGraphState *state;
    int n_poses, n_edges, chunks;
};

// Two kernels: a lane per edge (M, W r, chi2), then a lane per pose (b, the diagonal block and its factor).
hipError_t launch_pose_graph_linearize(const PoseGraphLinArgs &a, hipStream_t st);

// iter0 == 0: the start (x = 0, r = b, z, the first partials; the state words) in two kernels.  Then `iters` iterations of three
// kernels each - edges, poses, update - numbered iter0 .. iter0 + iters - 1, then one workgroup that brings the state words up to date.
hipError_t launch_pose_graph_pcg(const PoseGraphPcgArgs &a, int iter0, int iters, hipStream_t st);

}  // namespace sv
