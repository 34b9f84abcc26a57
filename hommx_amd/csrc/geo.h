// geo.h -- geometry / stencil descriptor shared by the kernel files of the blocked family.
#pragma once
#include <hip/hip_runtime.h>

namespace hommx {

typedef double d4 __attribute__((ext_vector_type(4)));

struct Geo {
  int dim, n, bs, t, kind, ncomp;
  int nn, npl, b, Bp, nsub, ncode, n_el;
  int voff[6][4][3];     // corner offset of local vertex a of sub-element s
  double grad[6][4][3];  // gradient of its P1 basis function on the unit-size cell (h = 1)
};

// in-plane neighbour q' of in-plane node q for in-plane code ipc
__device__ __forceinline__ int plane_neighbour(const Geo& G, int q, int ipc) {
  const int n = G.n;
  if (G.dim == 2) {
    const int o = ipc - 1;
    return (q + o + n) % n;
  }
  const int ox = ipc % 3 - 1, oy = ipc / 3 - 1;
  const int i = (q % n + ox + n) % n, j = (q / n + oy + n) % n;
  return i + n * j;
}

}  // namespace hommx
