// neighbors.hip -- padded neighbour index on the device.
// Replaces the host's O(N^2) Device::constructSiteNeighborList (Device.cpp:98-136) and the padding loop (:69-80):
// row i holds every j != i with site_dist(i, j) < nn_dist in ascending j, padded with -1 to the global maximum nn.
// Cell list with cells of edge >= nn_dist: O(N) work, same distance arithmetic as gpu_solvers.h:225-257, so the
// result is identical to the reference's (asserted against the oracle in tests/test_gpu_parity.py).
#include "cellgrid.h"

__global__ void k_minmax(int N, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z, double *out)
{
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * CELL_NT + threadIdx.x; i < N; i += gridDim.x * CELL_NT) {
        mn[0] = fmin(mn[0], x[i]); mx[0] = fmax(mx[0], x[i]);
        mn[1] = fmin(mn[1], y[i]); mx[1] = fmax(mx[1], y[i]);
        mn[2] = fmin(mn[2], z[i]); mx[2] = fmax(mx[2], z[i]);
    }
    block_box(mn, mx, out + blockIdx.x * 6);
}

__global__ void k_cell_scatter(int N, const int *__restrict__ cell_id, const int *__restrict__ cell_start, int *__restrict__ cell_fill,
                               int *__restrict__ cell_sites)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int c = cell_id[i];
    cell_sites[cell_start[c] + atomicAdd(&cell_fill[c], 1)] = i;     // order inside a cell is irrelevant: rows are sorted afterwards
}

// FILL = 0: count neighbours (row_cnt, global max); FILL = 1: write the row, sort it ascending, pad with -1
template <int FILL>
__global__ __launch_bounds__(128) void k_neigh(int N, CellGrid G, double nn_dist, const double *__restrict__ x, const double *__restrict__ y,
                                               const double *__restrict__ z, const int *__restrict__ cell_start, const int *__restrict__ cell_cnt,
                                               const int *__restrict__ cell_sites, int *__restrict__ max_nn, int nn, int *__restrict__ neigh)
{
    const int i = blockIdx.x * 128 + threadIdx.x;
    if (i >= N) return;
    const double xi = x[i], yi = y[i], zi = z[i];
    int cx, cy, cz; cell_of(G, xi, yi, zi, cx, cy, cz);
    int n = 0;
    int *row = FILL ? neigh + (size_t)i * nn : nullptr;
    for_each_neighbor_cell(G, cx, cy, cz, [&](int c) {
        const int s0 = cell_start[c], s1 = s0 + cell_cnt[c];
        for (int s = s0; s < s1; ++s) {
            const int j = cell_sites[s];
            if (j == i) continue;
            if (site_dist(xi, yi, zi, x[j], y[j], z[j], G.laty, G.latz, G.pbc) < nn_dist) {
                if (FILL) { if (n < nn) row[n] = j; }
                ++n;
            }
        }
    });
    if (!FILL) { atomicMax(max_nn, n); return; }
    const int cnt = min(n, nn);
    for (int a = 1; a < cnt; ++a) {                       // insertion sort of the thread's own row (<= nn entries)
        const int v = row[a]; int b = a - 1;
        while (b >= 0 && row[b] > v) { row[b + 1] = row[b]; --b; }
        row[b + 1] = v;
    }
    for (int a = cnt; a < nn; ++a) row[a] = -1;
}

// Two-call protocol: d_neigh_out == NULL computes the maximum neighbour count into *nn_out; the second call (same
// positions) fills d_neigh_out[N * nn] with nn = *nn_out.
extern "C" int dkmc_build_neighbor_index(int N, const double *d_x, const double *d_y, const double *d_z, const double *h_lattice,
                                         int pbc, double nn_dist, int *nn_out, int *d_neigh_out)
{
    Engine &e = eng(); hipStream_t st = e.stream;
    if (N <= 0) return dkmc_fail(13, "build_neighbor_index: no sites", __FILE__, __LINE__);
    // bounding box
    double *mm = (double *)scratch(S_MISC0, sizeof(double) * CELL_BOX_BLOCKS * 6);
    if (!mm) return e.err_code;
    hipLaunchKernelGGL(k_minmax, dim3(CELL_BOX_BLOCKS), dim3(CELL_NT), 0, st, N, d_x, d_y, d_z, mm);
    double h[CELL_BOX_BLOCKS * 6], mn[3], mx[3];
    HIPCHK(hipMemcpyAsync(h, mm, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    fold_boxes(h, mn, mx);
    // the non-periodic distance and binning never read laty, latz
    CellGrid G; G.pbc = pbc; G.laty = pbc ? h_lattice[1] : 1.0; G.latz = pbc ? h_lattice[2] : 1.0;
    G.x0 = mn[0]; G.y0 = mn[1]; G.z0 = mn[2];
    G.nx = (int)((mx[0] - mn[0]) / nn_dist) + 1; G.hx = nn_dist;
    if (pbc) {
        G.ny = (int)(G.laty / nn_dist); G.nz = (int)(G.latz / nn_dist);       // cells at least nn_dist wide
        if (G.ny < 3 || G.nz < 3) return dkmc_fail(14, "build_neighbor_index: periodic box narrower than 3 cells", __FILE__, __LINE__);
        G.hy = G.laty / G.ny; G.hz = G.latz / G.nz;
    } else {
        G.ny = (int)((mx[1] - mn[1]) / nn_dist) + 1; G.nz = (int)((mx[2] - mn[2]) / nn_dist) + 1; G.hy = G.hz = nn_dist;
    }
    const long long ncell = (long long)G.nx * G.ny * G.nz;
    if (ncell > (1ll << 30)) return dkmc_fail(15, "build_neighbor_index: too many cells", __FILE__, __LINE__);
    int *cell_id = (int *)scratch(S_AT_FLAG, (size_t)N * 4);
    int *cell_cnt = (int *)scratch(S_MISC1, (size_t)(ncell + 4) * 4 * 3);
    int *cell_sites = (int *)scratch(S_AT_SITE, (size_t)N * 4);
    int *mx_nn = (int *)scratch(S_MISC2, 16);
    if (!cell_id || !cell_cnt || !cell_sites || !mx_nn) return e.err_code;
    int *cell_start = cell_cnt + (ncell + 4), *cell_fill = cell_start + (ncell + 4);
    HIPCHK(hipMemsetAsync(cell_cnt, 0, (size_t)(ncell + 4) * 4 * 3, st));
    HIPCHK(hipMemsetAsync(mx_nn, 0, 16, st));
    const int gb = (N + CELL_NT - 1) / CELL_NT;
    hipLaunchKernelGGL(k_cell_count, dim3(gb), dim3(CELL_NT), 0, st, N, G, (const int *)nullptr, d_x, d_y, d_z, cell_id, cell_cnt);
    int rc = dkmc_exclusive_scan_i32(cell_cnt, cell_start, (int)ncell, nullptr); if (rc) return rc;
    hipLaunchKernelGGL(k_cell_scatter, dim3(gb), dim3(CELL_NT), 0, st, N, (const int *)cell_id, (const int *)cell_start, cell_fill, cell_sites);
    const int gn = (N + 127) / 128;
    if (!d_neigh_out) {
        hipLaunchKernelGGL((k_neigh<0>), dim3(gn), dim3(128), 0, st, N, G, nn_dist, d_x, d_y, d_z, (const int *)cell_start, (const int *)cell_cnt,
                           (const int *)cell_sites, mx_nn, 0, (int *)nullptr);
        KCHK();
        HIPCHK(hipMemcpyAsync(nn_out, mx_nn, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    hipLaunchKernelGGL((k_neigh<1>), dim3(gn), dim3(128), 0, st, N, G, nn_dist, d_x, d_y, d_z, (const int *)cell_start, (const int *)cell_cnt,
                       (const int *)cell_sites, mx_nn, *nn_out, d_neigh_out);
    KCHK();
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
