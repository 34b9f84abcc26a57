// struct_elem.h -- the micro elements of a structured plan, computed in the kernel (for_elements of elem_walk.h, k_assemble_loads of loads.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace hommx {

// Sub-simplices of a structured grid cell (hommx_amd/mesh.py: DiagonalType.right triangles, six tetrahedra around the v0-v7 diagonal):
// corner offset of local vertex a and its P1 gradient on the unit-size cell (h = 1: multiply by n)
__device__ constexpr int kOff2[2][3][2] = {{{0, 0}, {1, 0}, {1, 1}}, {{0, 0}, {0, 1}, {1, 1}}};
__device__ constexpr int kGrad2[2][3][2] = {{{-1, 0}, {1, -1}, {0, 1}}, {{0, -1}, {-1, 1}, {1, 0}}};
__device__ constexpr int kOff3[6][4][3] = {{{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 1, 1}}, {{0, 0, 0}, {1, 0, 0}, {1, 1, 1}, {1, 0, 1}},
                                           {{0, 0, 0}, {1, 0, 1}, {1, 1, 1}, {0, 0, 1}}, {{0, 0, 0}, {1, 1, 0}, {0, 1, 0}, {1, 1, 1}},
                                           {{0, 0, 0}, {0, 1, 1}, {0, 0, 1}, {1, 1, 1}}, {{0, 0, 0}, {0, 1, 0}, {0, 1, 1}, {1, 1, 1}}};
__device__ constexpr int kGrad3[6][4][3] = {{{-1, 0, 0}, {1, -1, 0}, {0, 1, -1}, {0, 0, 1}}, {{-1, 0, 0}, {1, 0, -1}, {0, 1, 0}, {0, -1, 1}},
                                            {{0, 0, -1}, {1, -1, 0}, {0, 1, 0}, {-1, 0, 1}}, {{0, -1, 0}, {1, 0, -1}, {-1, 1, 0}, {0, 0, 1}},
                                            {{0, 0, -1}, {-1, 1, 0}, {0, -1, 1}, {1, 0, 0}}, {{0, -1, 0}, {0, 1, -1}, {-1, 0, 1}, {1, 0, 0}}};

// periodic node and P1 gradient of vertex a of sub-simplex s of grid cell (i, j[, k]) on the n^dim grid (hn = n as a double)
template <int DIM>
__device__ __forceinline__ void struct_vertex(int i, int j, int k, int s, int a, int n, double hn, int& node, double (&g)[DIM]) {
  if constexpr (DIM == 2) {
    const int ii = i + kOff2[s][a][0], jj = j + kOff2[s][a][1];
    node = (ii == n ? 0 : ii) + n * (jj == n ? 0 : jj);
#pragma unroll
    for (int c = 0; c < 2; ++c) g[c] = kGrad2[s][a][c] * hn;
  } else {
    const int ii = i + kOff3[s][a][0], jj = j + kOff3[s][a][1], kk = k + kOff3[s][a][2];
    node = (ii == n ? 0 : ii) + n * ((jj == n ? 0 : jj) + n * (kk == n ? 0 : kk));
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = kGrad3[s][a][c] * hn;
  }
}

}  // namespace hommx
