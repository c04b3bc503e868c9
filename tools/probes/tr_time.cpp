// Developer probe: wall time of mi_csr_transpose_f32 at the C3 shape (uniform 105 non-zeros per row).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Imatrix-multiplication_amd/csrc tools/probes/tr_time.cpp matrix-multiplication_amd/csrc/csr_transpose_items.hip -o tools/probes/tr_time
#include "../../matrix-multiplication_amd/csrc/mi_status.hip"
#include "../../matrix-multiplication_amd/csrc/csr_transpose.hip"
#include <cstdio>
#include <random>
#include <vector>
#include <algorithm>
int main() {
  const int M = 1 << 20, K = 1 << 20, per = 105;
  std::mt19937_64 g(1);
  std::vector<int> rowptr(M + 1), col((size_t)M * per);
  std::vector<float> val((size_t)M * per, 1.f);
  for (int r = 0; r < M; ++r) {
    rowptr[r] = r * per;
    for (int j = 0; j < per; ++j) col[(size_t)r * per + j] = (int)(g() % K);
    std::sort(col.begin() + (size_t)r * per, col.begin() + (size_t)(r + 1) * per);
  }
  rowptr[M] = M * per;
  const long nnz = (long)M * per;
  int *d_rp, *d_col, *t_rp, *t_col; float *d_val, *t_val; void* ws;
  (void)hipMalloc(&d_rp, (M + 1) * 4); (void)hipMalloc(&d_col, nnz * 4); (void)hipMalloc(&d_val, nnz * 4);
  (void)hipMalloc(&t_rp, (K + 1) * 4); (void)hipMalloc(&t_col, nnz * 4); (void)hipMalloc(&t_val, nnz * 4);
  const size_t wsb = mi_csr_transpose_workspace_bytes(M, K, nnz);
  (void)hipMalloc(&ws, wsb);
  (void)hipMemcpy(d_rp, rowptr.data(), (M + 1) * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(d_col, col.data(), nnz * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(d_val, val.data(), nnz * 4, hipMemcpyHostToDevice);
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int it = 0; it < 4; ++it) {
    (void)hipEventRecord(e0);
    int st = mi_csr_transpose_f32(d_rp, d_col, d_val, nnz, M, K, t_rp, t_col, t_val, ws, wsb, nullptr);
    (void)hipEventRecord(e1);
    (void)hipDeviceSynchronize();
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    printf("status %d  %.3f ms\n", st, ms);
  }
  return 0;
}
