// cellgrid.h -- the one place that knows how points are binned into cells and how the cells around a point are walked (neighbors.hip: every
// site, cells of edge >= nn_dist; gaps.hip: the members only, cells of edge >= r_max).  A search that visits the cells for_each_neighbor_cell
// names sees every pair closer than the cell edge BECAUSE both sides bin with cell_of: change the two together, here.  How many cells a grid
// gets is the caller's decision (the index refuses a periodic box narrower than 3 cells, the gap analysis doubles the edge until the grid fits).
#pragma once
#include "common.h"

#define CELL_NT 256                  // threads of a workgroup in the kernels below ...
#define CELL_BOX_BLOCKS 256          // ... and the workgroups of a bounding-box pass = the partial boxes the host folds

struct CellGrid {
    double x0, y0, z0, hx, hy, hz;     // origin and cell edge per axis
    int nx, ny, nz, pbc;
    double laty, latz;
};

__device__ __forceinline__ void cell_of(const CellGrid &G, double x, double y, double z, int &cx, int &cy, int &cz)
{
    cx = (int)((x - G.x0) / G.hx);
    if (G.pbc) {                        // y, z are periodic: bin the wrapped coordinate
        double fy = y / G.laty; fy -= floor(fy);
        double fz = z / G.latz; fz -= floor(fz);
        cy = (int)(fy * G.ny); cz = (int)(fz * G.nz);
    } else { cy = (int)((y - G.y0) / G.hy); cz = (int)((z - G.z0) / G.hz); }
    cx = min(max(cx, 0), G.nx - 1); cy = min(max(cy, 0), G.ny - 1); cz = min(max(cz, 0), G.nz - 1);
}

// f(c) once for every distinct cell c next to (cx, cy, cz), the cell itself included: x outermost, then y, then z, offsets -1, 0, +1.  y and z
// wrap under pbc; a periodic axis with fewer than 3 cells is scanned whole, where the three offsets would name a cell twice.
template <class F>
__device__ __forceinline__ void for_each_neighbor_cell(const CellGrid &G, int cx, int cy, int cz, F f)
{
    const bool wy = G.pbc && G.ny < 3, wz = G.pbc && G.nz < 3;
    const int y0 = wy ? 0 : cy - 1, y1 = wy ? G.ny - 1 : cy + 1, z0 = wz ? 0 : cz - 1, z1 = wz ? G.nz - 1 : cz + 1;
    for (int ax = max(cx - 1, 0); ax <= min(cx + 1, G.nx - 1); ++ax)
        for (int qy = y0; qy <= y1; ++qy) {
            int ay = qy;
            if (G.pbc) ay = (ay + G.ny) % G.ny; else if (ay < 0 || ay >= G.ny) continue;
            for (int qz = z0; qz <= z1; ++qz) {
                int az = qz;
                if (G.pbc) az = (az + G.nz) % G.nz; else if (az < 0 || az >= G.nz) continue;
                f((ax * G.ny + ay) * G.nz + az);
            }
        }
}

// bounding box of a workgroup of CELL_NT threads: every thread brings the box of its own points, out6 receives {min x, y, z, max x, y, z}.
// Minima and maxima only: no order dependence.
__device__ __forceinline__ void block_box(const double mn[3], const double mx[3], double *out6)
{
    __shared__ double red[6][CELL_NT];
    const int t = threadIdx.x;
    for (int k = 0; k < 3; ++k) { red[k][t] = mn[k]; red[3 + k][t] = mx[k]; }
    __syncthreads();
    for (int s = CELL_NT / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < 3; ++k) { red[k][t] = fmin(red[k][t], red[k][t + s]); red[3 + k][t] = fmax(red[3 + k][t], red[3 + k][t + s]); }
        __syncthreads();
    }
    if (t < 6) out6[t] = red[t][0];
}

// the box of a pass of CELL_BOX_BLOCKS workgroups from their partial boxes, copied to the host
inline void fold_boxes(const double *h_box, double mn[3], double mx[3])
{
    for (int k = 0; k < 3; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; }
    for (int b = 0; b < CELL_BOX_BLOCKS; ++b)
        for (int k = 0; k < 3; ++k) { mn[k] = fmin(mn[k], h_box[b * 6 + k]); mx[k] = fmax(mx[k], h_box[b * 6 + 3 + k]); }
}

// cell of every site and the sites per cell.  label == null: every site is binned; else only the members, 0 <= label[i] < N, and the others get
// cell -1.  (Internal linkage: the header is compiled into more than one code object.)
static __global__ __launch_bounds__(CELL_NT) void k_cell_count(int N, CellGrid G, const int *__restrict__ label, const double *__restrict__ x,
                                                               const double *__restrict__ y, const double *__restrict__ z,
                                                               int *__restrict__ cell_id, int *__restrict__ cell_cnt)
{
    const int i = blockIdx.x * CELL_NT + threadIdx.x;
    if (i >= N) return;
    if (label && !(label[i] >= 0 && label[i] < N)) { cell_id[i] = -1; return; }
    int cx, cy, cz; cell_of(G, x[i], y[i], z[i], cx, cy, cz);
    const int c = (cx * G.ny + cy) * G.nz + cz;
    cell_id[i] = c;
    atomicAdd(&cell_cnt[c], 1);
}
