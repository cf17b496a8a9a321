// rx_isosurface.hip -- a triangle mesh of a uint8 volume by surface nets (host side postprocess/isosurface.py, whose
// surface_nets_numpy and counts_numpy are the statements).  One vertex per cell of the (Z+1, Y+1, X+1) grid whose corners are not all
// inside (value > level) or all outside, numbered in ascending linear cell index; one quad (two triangles) per lattice edge with one
// end inside, ordered by (owning cell, axis, first / second).  The output is a property of the volume alone: no slot is chosen by an
// atomic, there is no float atomic, and two runs give the same bytes.  The per-cell and per-edge arithmetic is rx_isosurface_core.h
// (shared with the host check); this file holds the kernels and the entry points.  Contraction is off and denormals are kept, so a
// position is the statement's float32, bit for bit.
//
// A workgroup (4 waves) owns a BAND of 4 cell planes x 8 cell rows and walks it along x in chunks of 64 cells.  The band reads
// 5 x 9 voxel rows; a wave loads a voxel row's 64 bytes of a chunk (lane = x) and the neighbours meet in LDS.
//
//   iso_classify_kernel  the ballot of `value > level` is a voxel row's 64 inside flags: 45 words + 45 halo bits in LDS per chunk.
//                        A thread per cell row of the band combines the eight words around it (iso_chunk_flags) into the chunk's
//                        active word -- written to `bits` -- and counts the active cells and the owned quads of its row.
//   iso_scan_*           exclusive prefix sums of both count columns over the cell rows, in int64: 1024 rows per workgroup scanned
//                        on their own, then the workgroup totals scanned by one workgroup, which leaves every base in its group's
//                        first word, then the base added to the rest.  Integers only: any order gives the same sums.
//   iso_emit_kernel      the bytes of the band's chunk in LDS (45 x 65).  A wave owns a cell row at a time, a lane a cell: its eight
//                        corners give the crossings again and the position (iso_vertex).  A cell's vertex id is its row's offset
//                        plus the active cells before it: a running popcount of the row's `bits` words before the chunk, kept in
//                        LDS for the band's 45 rows, plus the popcount of the word below the lane.  A quad's slot is its row's quad
//                        offset plus the ballots of the three crossing flags counted the same way.  Active lanes of a row write
//                        consecutive vertices and consecutive quads.
#include "rx_common.h"
#include "rx_isosurface_core.h"

#pragma clang fp contract(off)

#define RX_ISO_BLOCK 256
#define RX_ISO_WAVES (RX_ISO_BLOCK / 64)
#define RX_ISO_VY (RX_ISO_BJ + 1)
#define RX_ISO_SCAN_PER 4
#define RX_ISO_SCAN_GROUP (RX_ISO_BLOCK * RX_ISO_SCAN_PER)      // cell rows scanned by one workgroup
#define RX_ISO_SCAN_TOP 1024                                    // threads of the workgroup that scans the group totals
static_assert(RX_ISO_VROWS <= 64 && RX_ISO_BAND % RX_ISO_WAVES == 0, "one thread per band row; whole rows per wave");

// ---- classify -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_ISO_BLOCK) void iso_classify_kernel(const unsigned char* __restrict__ values, int level, int Z, int Y, int X,
                                                                    int k_lo, int k_hi, int nbj, uint64_t* __restrict__ bits,
                                                                    int2* __restrict__ row_counts) {
  __shared__ uint64_t s_b[RX_ISO_VROWS];
  __shared__ unsigned s_h[RX_ISO_VROWS];
  const int CZ = Z + 1, CY = Y + 1, CX = X + 1, W = (CX + 63) / 64;
  const int k0 = ((int)blockIdx.x / nbj) * RX_ISO_BK, j0 = ((int)blockIdx.x % nbj) * RX_ISO_BJ;      // inside the cell grid by the launch
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk = threadIdx.x / RX_ISO_BJ, jj = threadIdx.x % RX_ISO_BJ, k = k0 + kk, j = j0 + jj;
  const bool mine = threadIdx.x < RX_ISO_BAND && k < CZ && j < CY;      // this thread owns cell row (k, j)
  int nact = 0, nquad = 0;
  for (int ch = 0; ch < W; ++ch) {
    const int i0 = ch * 64, x = i0 + lane;
    for (int r = wave; r < RX_ISO_VROWS; r += RX_ISO_WAVES) {      // wave-uniform: the ballot sees 64 lanes
      const int z = k0 - 1 + r / RX_ISO_VY, y = j0 - 1 + r % RX_ISO_VY;
      bool in = false;
      unsigned h = 0;
      if (z >= 0 && z < Z && y >= 0 && y < Y) {      // only then is a byte read, at x < X
        const unsigned char* __restrict__ p = values + ((long)z * Y + y) * X;
        if (x < X) in = (int)p[x] > level;
        if (lane == 0 && i0 > 0) h = (int)p[i0 - 1] > level;      // i0 <= 64 * (W - 1) <= X
      }
      const unsigned long long m = __ballot(in);
      if (lane == 0) s_b[r] = m, s_h[r] = h;
    }
    __syncthreads();
    if (mine) {
      uint64_t act = 0, qz = 0, qy = 0, qx = 0;
      if (k >= k_lo && k < k_hi) {
        uint64_t b[4];
        unsigned halo = 0;
        for (int q = 0; q < 4; ++q) {
          const int r = (kk + (q >> 1)) * RX_ISO_VY + jj + (q & 1);
          b[q] = s_b[r], halo |= s_h[r] << q;
        }
        iso_chunk_flags(b, halo, &act, &qz, &qy, &qx);
      }
      bits[((long)k * CY + j) * W + ch] = act;
      nact += iso_popc(act), nquad += iso_popc(qz) + iso_popc(qy) + iso_popc(qx);
    }
    __syncthreads();
  }
  if (mine) row_counts[(long)k * CY + j] = make_int2(nact, nquad);
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------------------
struct iso_pair { long long v, q; };
__device__ __forceinline__ iso_pair operator+(iso_pair a, iso_pair b) { return iso_pair{a.v + b.v, a.q + b.q}; }

// exclusive scan of one value per thread over a workgroup of NW waves; `total` gets the workgroup's sum
template <int NW>
__device__ __forceinline__ iso_pair iso_block_scan(iso_pair x, iso_pair* s_w, iso_pair* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  iso_pair inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long v = __shfl_up(inc.v, o, 64), q = __shfl_up(inc.q, o, 64);
    if (lane >= o) inc.v += v, inc.q += q;
  }
  __syncthreads();      // s_w may still be read from the call before
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  iso_pair base{0, 0}, sum{0, 0};
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (w < wave) base = base + s_w[w];
    sum = sum + s_w[w];
  }
  *total = sum;
  return iso_pair{base.v + inc.v - x.v, base.q + inc.q - x.q};
}

__global__ __launch_bounds__(RX_ISO_BLOCK) void iso_scan_local_kernel(const int2* __restrict__ counts, long rows, longlong2* __restrict__ offs) {
  __shared__ iso_pair s_w[RX_ISO_WAVES];
  const long r0 = (long)blockIdx.x * RX_ISO_SCAN_GROUP + (long)threadIdx.x * RX_ISO_SCAN_PER;
  iso_pair c[RX_ISO_SCAN_PER], sum{0, 0}, total;
#pragma unroll
  for (int e = 0; e < RX_ISO_SCAN_PER; ++e) {
    c[e] = iso_pair{0, 0};
    if (r0 + e < rows) c[e] = iso_pair{counts[r0 + e].x, counts[r0 + e].y};
    sum = sum + c[e];
  }
  iso_pair at = iso_block_scan<RX_ISO_WAVES>(sum, s_w, &total);
#pragma unroll
  for (int e = 0; e < RX_ISO_SCAN_PER; ++e) {
    if (r0 + e < rows) offs[r0 + e] = make_longlong2(at.v, at.q);
    at = at + c[e];
  }
}

// one workgroup: group g's total is its last row's local offset + count; its base goes into its first row's word (local offset 0)
__global__ __launch_bounds__(RX_ISO_SCAN_TOP) void iso_scan_groups_kernel(const int2* __restrict__ counts, long rows, long groups,
                                                                          longlong2* offs, long long* __restrict__ totals) {
  __shared__ iso_pair s_w[RX_ISO_SCAN_TOP / 64];
  iso_pair carry{0, 0};
  for (long g0 = 0; g0 < groups; g0 += RX_ISO_SCAN_TOP) {      // uniform trip count
    const long g = g0 + threadIdx.x;
    iso_pair t{0, 0}, total;
    if (g < groups) {
      const long last = (g + 1) * RX_ISO_SCAN_GROUP < rows ? (g + 1) * RX_ISO_SCAN_GROUP - 1 : rows - 1;
      t = iso_pair{offs[last].x + counts[last].x, offs[last].y + counts[last].y};
    }
    const iso_pair at = iso_block_scan<RX_ISO_SCAN_TOP / 64>(t, s_w, &total);
    if (g < groups) offs[g * RX_ISO_SCAN_GROUP] = make_longlong2(carry.v + at.v, carry.q + at.q);      // read above by this thread alone
    carry = carry + total;
  }
  if (threadIdx.x == 0) totals[0] = carry.v, totals[1] = carry.q;
}

__global__ __launch_bounds__(RX_ISO_BLOCK) void iso_scan_add_kernel(long rows, longlong2* offs) {
  const long r = (long)blockIdx.x * RX_ISO_BLOCK + threadIdx.x;
  if (r >= rows || r % RX_ISO_SCAN_GROUP == 0) return;      // a group's first word holds the base and is only read here
  const longlong2 base = offs[r - r % RX_ISO_SCAN_GROUP];
  longlong2 o = offs[r];
  o.x += base.x, o.y += base.y;
  offs[r] = o;
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_ISO_BLOCK) void iso_emit_kernel(const unsigned char* __restrict__ values, int level, int Z, int Y, int X,
                                                                int z_base, int nbj, int bk0, const uint64_t* __restrict__ bits,
                                                                const longlong2* __restrict__ offs, int k_emit, long long v_skip,
                                                                long long q_skip, long long vertex_base, long long nv, long long nq,
                                                                float* __restrict__ vertices, long long* __restrict__ triangles) {
  __shared__ unsigned char s_v[RX_ISO_VROWS][68];      // [r][0]: x = i0 - 1, [r][1 + l]: x = i0 + l
  __shared__ uint64_t s_word[RX_ISO_VROWS];            // cell row (k0 - 1 + r / 9, j0 - 1 + r % 9): its `bits` word of this chunk,
  __shared__ int s_run[RX_ISO_VROWS];                  // its active cells before the chunk,
  __shared__ long long s_voff[RX_ISO_VROWS], s_qoff[RX_ISO_VROWS];      // its scanned offsets
  const int CZ = Z + 1, CY = Y + 1, CX = X + 1, W = (CX + 63) / 64;
  const int k0 = (bk0 + (int)blockIdx.x / nbj) * RX_ISO_BK, j0 = ((int)blockIdx.x % nbj) * RX_ISO_BJ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long crow = -1;      // threads 0 .. 44: the cell row they keep the words of, -1 outside the grid
  if (threadIdx.x < RX_ISO_VROWS) {
    const int kc = k0 - 1 + (int)threadIdx.x / RX_ISO_VY, jc = j0 - 1 + (int)threadIdx.x % RX_ISO_VY;
    if (kc >= 0 && kc < CZ && jc >= 0 && jc < CY) crow = (long)kc * CY + jc;
    s_voff[threadIdx.x] = crow >= 0 ? offs[crow].x : 0;
    s_qoff[threadIdx.x] = crow >= 0 ? offs[crow].y : 0;
    s_run[threadIdx.x] = 0;
    s_word[threadIdx.x] = 0;
  }
  int qrun[RX_ISO_BAND / RX_ISO_WAVES];      // the quads of this wave's rows before the chunk
#pragma unroll
  for (int it = 0; it < RX_ISO_BAND / RX_ISO_WAVES; ++it) qrun[it] = 0;

  for (int ch = 0; ch < W; ++ch) {
    const int i0 = ch * 64, x = i0 + lane;
    for (int r = wave; r < RX_ISO_VROWS; r += RX_ISO_WAVES) {
      const int z = k0 - 1 + r / RX_ISO_VY, y = j0 - 1 + r % RX_ISO_VY;
      unsigned char b = 0, h = 0;
      if (z >= 0 && z < Z && y >= 0 && y < Y) {      // only then is a byte read, at x < X
        const unsigned char* __restrict__ p = values + ((long)z * Y + y) * X;
        if (x < X) b = p[x];
        if (lane == 0 && i0 > 0) h = p[i0 - 1];
      }
      s_v[r][1 + lane] = b;
      if (lane == 0) s_v[r][0] = h;
    }
    if (threadIdx.x < RX_ISO_VROWS) {      // nobody else touches these two words between the barriers
      s_run[threadIdx.x] += iso_popc(s_word[threadIdx.x]);
      s_word[threadIdx.x] = crow >= 0 ? bits[crow * W + ch] : 0ull;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RX_ISO_BAND / RX_ISO_WAVES; ++it) {
      const int rr = it * RX_ISO_WAVES + wave, kk = rr / RX_ISO_BJ, jj = rr % RX_ISO_BJ, k = k0 + kk, j = j0 + jj;
      if (k >= CZ || j >= CY || k < k_emit) continue;      // wave-uniform
      const int r = (kk + 1) * RX_ISO_VY + jj + 1, rJ = r - 1, rK = r - RX_ISO_VY, rKJ = rK - 1;
      const uint64_t word = s_word[r];
      if (word == 0ull) continue;      // wave-uniform: no active cell in this chunk of the row, so no vertex and no quad
      const bool act = (word >> lane) & 1ull;
      unsigned char c[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) c[q] = s_v[(kk + (q >> 2)) * RX_ISO_VY + jj + ((q >> 1) & 1)][lane + (q & 1)];
      const bool in0 = (int)c[0] > level;
      const bool cz = act && ((int)c[4] > level) != in0, cy = act && ((int)c[2] > level) != in0, cx = act && ((int)c[1] > level) != in0;
      const unsigned long long bz = __ballot(cz), by = __ballot(cy), bx = __ballot(cx);
      const long long pC = s_voff[r] + s_run[r] + iso_prefix(word, lane);
      if (act) {
        float p[3];
        iso_vertex(c, level, k - 1 + z_base, j - 1, x - 1, p);
        const long long slot = pC - v_skip;
        if (slot >= 0 && slot < nv) vertices[3 * slot] = p[0], vertices[3 * slot + 1] = p[1], vertices[3 * slot + 2] = p[2];
        if (cz || cy || cx) {
          const long long pJ = s_voff[rJ] + s_run[rJ] + iso_prefix(s_word[rJ], lane);
          const long long pK = s_voff[rK] + s_run[rK] + iso_prefix(s_word[rK], lane);
          const long long pKJ = s_voff[rKJ] + s_run[rKJ] + iso_prefix(s_word[rKJ], lane);
          long long qs = s_qoff[r] + qrun[it] + iso_prefix(bz, lane) + iso_prefix(by, lane) + iso_prefix(bx, lane) - q_skip;
#pragma unroll
          for (int slot3 = 0; slot3 < 3; ++slot3) {
            if (!(slot3 == 0 ? cz : slot3 == 1 ? cy : cx)) continue;
            int64_t t[6];
            iso_quad(slot3, in0, pC, pJ, pK, pKJ, t);
            if (qs >= 0 && qs < nq) {
#pragma unroll
              for (int e = 0; e < 6; ++e) triangles[6 * qs + e] = vertex_base + t[e];
            }
            ++qs;
          }
        }
      }
      qrun[it] += iso_popc(bz) + iso_popc(by) + iso_popc(bx);
    }
    __syncthreads();
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
static inline int iso_shape_ok(const char* fn, int level, int z, int y, int x) {
  if (z <= 0 || y <= 0 || x <= 0) RX_FAIL(RX_EINVAL, "%s: sizes must be positive (got z=%d y=%d x=%d)", fn, z, y, x);
  if (level < 0 || level > 254) RX_FAIL(RX_EINVAL, "%s: level %d (0 .. 254: inside is value > level)", fn, level);
  if (z > RX_ISO_MAX_EXTENT || y > RX_ISO_MAX_EXTENT || x > RX_ISO_MAX_EXTENT)
    RX_FAIL(RX_EINVAL, "%s: an extent of 2^24 - 2 or more (z=%d y=%d x=%d): a position must be an exact float32 integer plus a fraction", fn, z, y, x);
  // (z+1)(y+1) first: each factor is below 2^24 + 1, so the product fits a long; then the division keeps the third step from overflowing
  const long zy = (long)(z + 1) * (y + 1);
  if (zy > RX_ISO_MAX_CELLS || zy > RX_ISO_MAX_CELLS / (x + 1))
    RX_FAIL(RX_EINVAL, "%s: more than 2^31 - 2 cells in a volume of z=%d y=%d x=%d", fn, z, y, x);
  // one workgroup of 256 threads per band of 4 x 8 cell rows: a launch holds fewer than 2^32 threads, so at most 2^24 - 1 bands
  const long bands = (long)((z + 1 + RX_ISO_BK - 1) / RX_ISO_BK) * ((y + 1 + RX_ISO_BJ - 1) / RX_ISO_BJ);
  if (bands > RX_ISO_MAX_BANDS)
    RX_FAIL(RX_EINVAL, "%s: %ld bands of %d x %d cell rows in a volume of z=%d y=%d (at most 2^24 - 1 in a launch: run it in slabs of planes)", fn,
            bands, RX_ISO_BK, RX_ISO_BJ, z, y);
  return RX_OK;
}

extern "C" int rx_iso_classify(const uint8_t* values, int level, int z, int y, int x, int k_lo, int k_hi, uint64_t* bits, int32_t* row_counts,
                               void* stream) {
  if (!values) RX_FAIL(RX_EINVAL, "rx_iso_classify: null input pointer");
  if (!bits || !row_counts) RX_FAIL(RX_EINVAL, "rx_iso_classify: null output pointer");
  if (int rc = iso_shape_ok("rx_iso_classify", level, z, y, x)) return rc;
  if (k_lo < 0 || k_hi > z + 1 || k_lo > k_hi) RX_FAIL(RX_EINVAL, "rx_iso_classify: cell planes [%d, %d) of 0 .. %d", k_lo, k_hi, z + 1);
  if ((((uintptr_t)bits | (uintptr_t)row_counts) & 7) != 0) RX_FAIL(RX_EINVAL, "rx_iso_classify: bits and row_counts must be 8-byte aligned");
  const int nbj = (y + 1 + RX_ISO_BJ - 1) / RX_ISO_BJ, nbk = (z + 1 + RX_ISO_BK - 1) / RX_ISO_BK;      // nbj * nbk <= RX_ISO_MAX_BANDS (iso_shape_ok)
  hipLaunchKernelGGL(iso_classify_kernel, dim3((unsigned)(nbj * nbk)), dim3(RX_ISO_BLOCK), 0, (hipStream_t)stream, values, level, z, y, x, k_lo,
                     k_hi, nbj, bits, (int2*)row_counts);
  RX_CHECK_LAUNCH("rx_iso_classify");
  return RX_OK;
}

extern "C" int rx_iso_scan(const int32_t* row_counts, long rows, int64_t* row_offsets, int64_t* totals, void* stream) {
  if (!row_counts) RX_FAIL(RX_EINVAL, "rx_iso_scan: null input pointer");
  if (!row_offsets || !totals) RX_FAIL(RX_EINVAL, "rx_iso_scan: null output pointer");
  if (rows <= 0 || rows > RX_ISO_MAX_CELLS) RX_FAIL(RX_EINVAL, "rx_iso_scan: %ld cell rows (1 .. 2^31 - 2)", rows);
  if (((uintptr_t)row_counts & 7) != 0 || ((uintptr_t)row_offsets & 15) != 0 || ((uintptr_t)totals & 7) != 0)
    RX_FAIL(RX_EINVAL, "rx_iso_scan: row_counts and totals must be 8-byte aligned, row_offsets 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long groups = (rows + RX_ISO_SCAN_GROUP - 1) / RX_ISO_SCAN_GROUP;
  hipLaunchKernelGGL(iso_scan_local_kernel, dim3((unsigned)groups), dim3(RX_ISO_BLOCK), 0, st, (const int2*)row_counts, rows, (longlong2*)row_offsets);
  RX_CHECK_LAUNCH("rx_iso_scan");
  hipLaunchKernelGGL(iso_scan_groups_kernel, dim3(1), dim3(RX_ISO_SCAN_TOP), 0, st, (const int2*)row_counts, rows, groups, (longlong2*)row_offsets,
                     (long long*)totals);
  RX_CHECK_LAUNCH("rx_iso_scan");
  if (groups > 1) {
    hipLaunchKernelGGL(iso_scan_add_kernel, dim3((unsigned)((rows + RX_ISO_BLOCK - 1) / RX_ISO_BLOCK)), dim3(RX_ISO_BLOCK), 0, st, rows,
                       (longlong2*)row_offsets);
    RX_CHECK_LAUNCH("rx_iso_scan");
  }
  return RX_OK;
}

extern "C" int rx_iso_emit(const uint8_t* values, int level, int z, int y, int x, int z_base, const uint64_t* bits, const int64_t* row_offsets,
                           int k_emit, int64_t v_skip, int64_t q_skip, int64_t vertex_base, int64_t n_vertices, int64_t n_quads,
                           float* vertices, int64_t* triangles, void* stream) {
  if (!values || !bits || !row_offsets) RX_FAIL(RX_EINVAL, "rx_iso_emit: null input pointer");
  if ((n_vertices > 0 && !vertices) || (n_quads > 0 && !triangles)) RX_FAIL(RX_EINVAL, "rx_iso_emit: null output pointer");
  if (int rc = iso_shape_ok("rx_iso_emit", level, z, y, x)) return rc;
  if (z_base < 0 || z_base > RX_ISO_MAX_EXTENT - z)
    RX_FAIL(RX_EINVAL, "rx_iso_emit: z_base %d: plane %d + %d is 2^24 - 2 or more", z_base, z_base, z);
  if (k_emit < 0 || k_emit > z + 1) RX_FAIL(RX_EINVAL, "rx_iso_emit: k_emit %d (0 .. %d)", k_emit, z + 1);
  if (n_vertices < 0 || n_quads < 0 || v_skip < 0 || q_skip < 0) RX_FAIL(RX_EINVAL, "rx_iso_emit: negative counts");
  if ((((uintptr_t)bits | (uintptr_t)triangles) & 7) != 0 || ((uintptr_t)row_offsets & 15) != 0 || ((uintptr_t)vertices & 3) != 0)
    RX_FAIL(RX_EINVAL, "rx_iso_emit: misaligned pointer");
  const int nbj = (y + 1 + RX_ISO_BJ - 1) / RX_ISO_BJ, nbk = (z + 1 + RX_ISO_BK - 1) / RX_ISO_BK, bk0 = k_emit / RX_ISO_BK;
  if (bk0 >= nbk || (n_vertices == 0 && n_quads == 0)) return RX_OK;      // nothing to write
  hipLaunchKernelGGL(iso_emit_kernel, dim3((unsigned)(nbj * (nbk - bk0))), dim3(RX_ISO_BLOCK), 0, (hipStream_t)stream, values, level, z, y, x,
                     z_base, nbj, bk0, bits, (const longlong2*)row_offsets, k_emit, (long long)v_skip, (long long)q_skip, (long long)vertex_base,
                     (long long)n_vertices, (long long)n_quads, vertices, (long long*)triangles);
  RX_CHECK_LAUNCH("rx_iso_emit");
  return RX_OK;
}
