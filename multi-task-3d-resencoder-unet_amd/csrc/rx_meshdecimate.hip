// rx_meshdecimate.hip -- decimation of an indexed triangle mesh by vertex clustering on a uniform grid, on the device (host side
// postprocess/decimate.py, whose decimate_numpy is the statement).  The per-vertex, per-cluster and per-triangle work is
// rx_meshdecimate_core.h (shared with the host check); this file holds the kernels and the entry points.  Contraction is off and
// denormals are kept, so a representative is the statement's float32, bit for bit.  There is no float atomic anywhere, and every
// number that leaves here is derived from cell keys and smallest member ids, never from which thread came first.  The prefix sums
// between the passes are rx_mesh_scan (rx_meshrefine.hip).
//
//   md_keys_kernel       a thread per vertex: its cell key; a cell index outside (-2^20, 2^20) raises bit 0 of the flag.
//   md_insert_kernel     a thread per vertex: finds or claims its key's slot in the open-addressing table (64-bit compare-and-swap,
//                        linear probing, at most `capacity` probes: exhaustion raises bit 1 of the flag, nothing spins) and lowers
//                        the slot's smallest id with an integer atomic minimum.
//   md_first_kernel      a thread per vertex: first[v] = v is the smallest id of its slot.  The scan of `first` numbers the clusters
//                        by ascending smallest member.
//   md_number_kernel     a thread per vertex: cluster_of[v] = scan[smallest id of its slot].
//   md_count_kernel      a thread per vertex: one integer atomic add into its cluster's member count.
//   md_fill_kernel       a thread per vertex: takes the next slot of its cluster's member list at a cursor.  Arrival chooses the slot.
//   md_mean_kernel       a thread per cluster: heap sort of its member list in place (any size: the list lives in global memory),
//                        then the sum in list order and the division.  After the sort nothing of the arrival order is left.
//   md_nearest_kernel    a thread per vertex: an integer atomic minimum of (bits of d) << 32 | id on its cluster's word.
//   md_pick_kernel       a thread per cluster: copies the winner's position.
//   md_remap_kernel      a thread per triangle: a triangle with three different clusters marks them referenced and counts itself
//                        at its smallest cluster.
//   md_attach_kernel     a thread per triangle: stores (middle, largest, triangle) at its smallest cluster's cursor.
//   md_unique_kernel     a thread per cluster: heap sort of its entries in place, keep flag for the first entry of each
//                        (middle, largest) run, which is the lowest triangle index.
//   md_emit_*            a thread per triangle / per cluster: kept triangles renumbered at the scan of the keep flags, referenced
//                        clusters' representatives at the scan of the referenced flags.
#include "rx_common.h"
#include "rx_meshdecimate_core.h"
#include "rx_mesh_host.h"

#pragma clang fp contract(off)

// ---- clusters ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_MESH_BLOCK) void md_keys_kernel(const float* __restrict__ pos, long long V, float cell, long long* __restrict__ keys,
                                                              int* __restrict__ flag) {
  RX_MESH_THREAD(v, V);
  const float p[3] = {pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]};
  int64_t key = MD_EMPTY;
  if (!md_key(p, cell, &key)) atomicOr(flag, 1);
  keys[v] = key;
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_insert_kernel(const long long* __restrict__ keys, long long V, long long capacity,
                                                                long long* table_keys, unsigned* table_min, int* __restrict__ slot_of,
                                                                int* __restrict__ flag) {
  RX_MESH_THREAD(v, V);
  const long long key = keys[v];
  int32_t slot = -1;
  if (key >= 0) {      // a vertex outside the key range has no key
    slot = md_insert(key, (int32_t)v, capacity, (int64_t*)table_keys, table_min);
    if (slot < 0) atomicOr(flag, 2);
  }
  slot_of[v] = slot;
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_first_kernel(long long V, const int* __restrict__ slot_of, long long capacity,
                                                               const unsigned* __restrict__ table_min, int* __restrict__ first) {
  RX_MESH_THREAD(v, V);
  first[v] = md_smallest(slot_of[v], capacity, table_min, V) == (int32_t)v;
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_number_kernel(long long V, const int* __restrict__ slot_of, long long capacity,
                                                                const unsigned* __restrict__ table_min, const long long* __restrict__ rank,
                                                                long long* __restrict__ cluster_of) {
  RX_MESH_THREAD(v, V);
  const int32_t m = md_smallest(slot_of[v], capacity, table_min, V);
  cluster_of[v] = m < 0 ? -1 : rank[m];
}

// ---- representatives --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_MESH_BLOCK) void md_count_kernel(const long long* __restrict__ cluster_of, long long V, long long C,
                                                               int* __restrict__ counts) {
  RX_MESH_THREAD(v, V);
  const long long c = cluster_of[v];
  if ((unsigned long long)c < (unsigned long long)C) atomicAdd(&counts[c], 1);
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_fill_kernel(const long long* __restrict__ cluster_of, long long V, long long C,
                                                              const long long* __restrict__ moff, int* __restrict__ cursor, long long capacity,
                                                              int* __restrict__ members) {
  RX_MESH_THREAD(v, V);
  const long long c = cluster_of[v];
  if ((unsigned long long)c >= (unsigned long long)C) return;
  const long long b = moff[c], e = moff[c + 1];
  const long long at = b + atomicAdd(&cursor[c], 1);
  if (at >= 0 && at < e && at < capacity) members[at] = (int)v;      // at >= e: more members than were counted -- not this mesh's scan
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_mean_kernel(const float* __restrict__ pos, long long V, long long C,
                                                              const long long* __restrict__ moff, int* members, long long capacity,
                                                              float* __restrict__ reps) {
  RX_MESH_THREAD(c, C);
  long long b = moff[c], e = moff[c + 1];
  if (b < 0 || e > capacity || e < b) b = e = 0;      // not a scan of this mesh: the cluster gets nothing
  float r[3] = {0.0f, 0.0f, 0.0f};
  if (e > b) md_mean(members + b, e - b, pos, V, r);
  reps[3 * c] = r[0], reps[3 * c + 1] = r[1], reps[3 * c + 2] = r[2];
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_nearest_kernel(const float* __restrict__ pos, const long long* __restrict__ keys, long long V,
                                                                 float cell, const long long* __restrict__ cluster_of, long long C,
                                                                 unsigned long long* __restrict__ best) {
  RX_MESH_THREAD(v, V);
  const long long c = cluster_of[v];
  if ((unsigned long long)c >= (unsigned long long)C || keys[v] < 0) return;
  const float p[3] = {pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]};
  atomicMin(&best[c], (unsigned long long)md_nearest_pack(p, keys[v], cell, (int32_t)v));
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_pick_kernel(const float* __restrict__ pos, long long V, long long C,
                                                              const unsigned long long* __restrict__ best, float* __restrict__ reps) {
  RX_MESH_THREAD(c, C);
  const unsigned long long m = best[c] & 0xffffffffULL;
  const bool ok = best[c] != ~0ULL && m < (unsigned long long)V;
  for (int k = 0; k < 3; ++k) reps[3 * c + k] = ok ? pos[3 * m + k] : 0.0f;
}

// ---- triangles --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_MESH_BLOCK) void md_remap_kernel(const long long* __restrict__ tri, long long T, long long V,
                                                               const long long* __restrict__ cluster_of, long long C, int* __restrict__ counts,
                                                               int* __restrict__ used, int* __restrict__ flag) {
  RX_MESH_THREAD(t, T);
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  if (!mr_triangle_ok(id, V)) {
    atomicOr(flag, 4);
    return;
  }
  int64_t c[3];
  int32_t lo, mid, hi;
  if (!md_remap(id, V, (const int64_t*)cluster_of, C, c, &lo, &mid, &hi)) return;
  used[lo] = 1, used[mid] = 1, used[hi] = 1;      // every writer stores the same value
  atomicAdd(&counts[lo], 1);
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_attach_kernel(const long long* __restrict__ tri, long long T, long long V,
                                                                const long long* __restrict__ cluster_of, long long C,
                                                                const long long* __restrict__ toff, int* __restrict__ cursor, long long capacity,
                                                                int* __restrict__ entries) {
  RX_MESH_THREAD(t, T);
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  int64_t c[3];
  int32_t lo, mid, hi;
  if (!md_remap(id, V, (const int64_t*)cluster_of, C, c, &lo, &mid, &hi)) return;
  const long long b = toff[lo], e = toff[lo + 1];
  const long long at = b + atomicAdd(&cursor[lo], 1);
  if (at < 0 || at >= e || at >= capacity) return;
  entries[3 * at] = mid, entries[3 * at + 1] = hi, entries[3 * at + 2] = (int)t;
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_unique_kernel(long long C, const long long* __restrict__ toff, long long capacity, int* entries,
                                                                long long T, int* __restrict__ keep) {
  RX_MESH_THREAD(c, C);
  const long long b = toff[c], e = toff[c + 1];
  if (b < 0 || e > capacity || e <= b) return;
  md_unique(entries + 3 * b, e - b, T, keep);
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_emit_triangles_kernel(const long long* __restrict__ tri, long long T, long long V,
                                                                        const long long* __restrict__ cluster_of, long long C,
                                                                        const int* __restrict__ keep, const long long* __restrict__ koff,
                                                                        const long long* __restrict__ uoff, long long capacity,
                                                                        long long* __restrict__ out) {
  RX_MESH_THREAD(t, T);
  if (!keep[t]) return;
  const long long at = koff[t];
  if (at < 0 || at >= capacity) return;
  for (int k = 0; k < 3; ++k) {
    const long long id = tri[3 * t + k];
    const long long c = (unsigned long long)id < (unsigned long long)V ? cluster_of[id] : -1;
    out[3 * at + k] = (unsigned long long)c < (unsigned long long)C ? uoff[c] : -1;
  }
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void md_emit_vertices_kernel(long long C, const int* __restrict__ used, const long long* __restrict__ uoff,
                                                                       const float* __restrict__ reps, long long capacity, float* __restrict__ out) {
  RX_MESH_THREAD(c, C);
  if (!used[c]) return;
  const long long at = uoff[c];
  if (at < 0 || at >= capacity) return;
  out[3 * at] = reps[3 * c], out[3 * at + 1] = reps[3 * c + 1], out[3 * at + 2] = reps[3 * c + 2];
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------
static inline int md_cell_ok(const char* fn, float cell) {
  if (!(cell > 0.0f && cell <= 3.402823466e38f)) RX_FAIL(RX_EINVAL, "%s: cell must be finite and > 0", fn);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_keys(const float* vertices, int64_t n_vertices, float cell, int64_t* keys, int32_t* flag, void* stream) {
  const char* fn = "rx_mesh_cluster_keys";
  if (!vertices) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!keys || !flag) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  if (int rc = md_cell_ok(fn, cell)) return rc;
  if (!RX_MESH_ALIGNED(vertices, 4) || !RX_MESH_ALIGNED(keys, 8) || !RX_MESH_ALIGNED(flag, 4)) RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  RX_MESH_LAUNCH(fn, md_keys_kernel, n_vertices, stream, vertices, (long long)n_vertices, cell, (long long*)keys, flag);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_assign(const int64_t* keys, int64_t n_vertices, int64_t capacity, int64_t* table_keys, int32_t* table_min,
                                      int32_t* slot_of, int32_t* first, int32_t* flag, void* stream) {
  const char* fn = "rx_mesh_cluster_assign";
  if (!keys) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!table_keys || !table_min || !slot_of || !first || !flag) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  if (capacity <= n_vertices || capacity > (1LL << 31) || (capacity & (capacity - 1)) != 0)
    RX_FAIL(RX_EINVAL, "%s: table capacity %lld (a power of two above the %lld vertices, at most 2^31)", fn, (long long)capacity, (long long)n_vertices);
  if (!RX_MESH_ALIGNED(keys, 8) || !RX_MESH_ALIGNED(table_keys, 8) || !RX_MESH_ALIGNED(table_min, 4) || !RX_MESH_ALIGNED(slot_of, 4) || !RX_MESH_ALIGNED(first, 4) ||
      !RX_MESH_ALIGNED(flag, 4))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(table_keys, 0xff, (size_t)capacity * 8, st) != hipSuccess ||      // MD_EMPTY
      hipMemsetAsync(table_min, 0xff, (size_t)capacity * 4, st) != hipSuccess)         // MD_NO_MIN
    RX_FAIL(RX_ELAUNCH, "%s: clearing the table failed", fn);
  RX_MESH_LAUNCH(fn, md_insert_kernel, n_vertices, st, (const long long*)keys, (long long)n_vertices, (long long)capacity, (long long*)table_keys,
            (unsigned*)table_min, slot_of, flag);
  RX_MESH_LAUNCH(fn, md_first_kernel, n_vertices, st, (long long)n_vertices, (const int*)slot_of, (long long)capacity, (const unsigned*)table_min, first);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_number(int64_t n_vertices, const int32_t* slot_of, int64_t capacity, const int32_t* table_min, const int64_t* rank,
                                      int64_t* cluster_of, void* stream) {
  const char* fn = "rx_mesh_cluster_number";
  if (!slot_of || !table_min || !rank) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!cluster_of) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  if (capacity <= n_vertices || capacity > (1LL << 31)) RX_FAIL(RX_EINVAL, "%s: table capacity %lld", fn, (long long)capacity);
  if (!RX_MESH_ALIGNED(slot_of, 4) || !RX_MESH_ALIGNED(table_min, 4) || !RX_MESH_ALIGNED(rank, 8) || !RX_MESH_ALIGNED(cluster_of, 8))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  RX_MESH_LAUNCH(fn, md_number_kernel, n_vertices, stream, (long long)n_vertices, slot_of, (long long)capacity, (const unsigned*)table_min, (const long long*)rank,
            (long long*)cluster_of);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_count(const int64_t* cluster_of, int64_t n_vertices, int64_t n_clusters, int32_t* counts, void* stream) {
  const char* fn = "rx_mesh_cluster_count";
  if (!cluster_of) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!counts) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  RX_MESH_CLUSTERS(fn, n_clusters, n_vertices);
  if (!RX_MESH_ALIGNED(cluster_of, 8) || !RX_MESH_ALIGNED(counts, 4)) RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)n_clusters * 4, st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "%s: clearing the counts failed", fn);
  RX_MESH_LAUNCH(fn, md_count_kernel, n_vertices, st, (const long long*)cluster_of, (long long)n_vertices, (long long)n_clusters, counts);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_fill(const int64_t* cluster_of, int64_t n_vertices, int64_t n_clusters, const int64_t* member_offsets, int32_t* cursor,
                                    int64_t capacity, int32_t* members, void* stream) {
  const char* fn = "rx_mesh_cluster_fill";
  if (!cluster_of || !member_offsets) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!cursor || !members) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  RX_MESH_CLUSTERS(fn, n_clusters, n_vertices);
  if (capacity < 0 || capacity > RX_MESH_MAX_VERTICES) RX_FAIL(RX_EINVAL, "%s: capacity %lld (0 .. 2^31 - 2 members)", fn, (long long)capacity);
  if (!RX_MESH_ALIGNED(cluster_of, 8) || !RX_MESH_ALIGNED(member_offsets, 8) || !RX_MESH_ALIGNED(cursor, 4) || !RX_MESH_ALIGNED(members, 4))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(cursor, 0, (size_t)n_clusters * 4, st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "%s: clearing the cursors failed", fn);
  RX_MESH_LAUNCH(fn, md_fill_kernel, n_vertices, st, (const long long*)cluster_of, (long long)n_vertices, (long long)n_clusters,
            (const long long*)member_offsets, cursor, (long long)capacity, members);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_mean(const float* vertices, int64_t n_vertices, int64_t n_clusters, const int64_t* member_offsets, int32_t* members,
                                    int64_t capacity, float* representatives, void* stream) {
  const char* fn = "rx_mesh_cluster_mean";
  if (!vertices || !member_offsets || !members) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!representatives) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  RX_MESH_CLUSTERS(fn, n_clusters, n_vertices);
  if (capacity < 0 || capacity > RX_MESH_MAX_VERTICES) RX_FAIL(RX_EINVAL, "%s: capacity %lld (0 .. 2^31 - 2 members)", fn, (long long)capacity);
  if (!RX_MESH_ALIGNED(vertices, 4) || !RX_MESH_ALIGNED(member_offsets, 8) || !RX_MESH_ALIGNED(members, 4) || !RX_MESH_ALIGNED(representatives, 4))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  RX_MESH_LAUNCH(fn, md_mean_kernel, n_clusters, stream, vertices, (long long)n_vertices, (long long)n_clusters, (const long long*)member_offsets, members,
            (long long)capacity, representatives);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_nearest(const float* vertices, const int64_t* keys, int64_t n_vertices, float cell, const int64_t* cluster_of,
                                       int64_t n_clusters, uint64_t* best, float* representatives, void* stream) {
  const char* fn = "rx_mesh_cluster_nearest";
  if (!vertices || !keys || !cluster_of) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!best || !representatives) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  RX_MESH_CLUSTERS(fn, n_clusters, n_vertices);
  if (int rc = md_cell_ok(fn, cell)) return rc;
  if (!RX_MESH_ALIGNED(vertices, 4) || !RX_MESH_ALIGNED(keys, 8) || !RX_MESH_ALIGNED(cluster_of, 8) || !RX_MESH_ALIGNED(best, 8) || !RX_MESH_ALIGNED(representatives, 4))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(best, 0xff, (size_t)n_clusters * 8, st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "%s: clearing the minima failed", fn);
  RX_MESH_LAUNCH(fn, md_nearest_kernel, n_vertices, st, vertices, (const long long*)keys, (long long)n_vertices, cell, (const long long*)cluster_of,
            (long long)n_clusters, (unsigned long long*)best);
  RX_MESH_LAUNCH(fn, md_pick_kernel, n_clusters, st, vertices, (long long)n_vertices, (long long)n_clusters, (const unsigned long long*)best,
            representatives);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_remap(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* cluster_of, int64_t n_clusters,
                                     int32_t* counts, int32_t* used, int32_t* flag, void* stream) {
  const char* fn = "rx_mesh_cluster_remap";
  if (!triangles || !cluster_of) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!counts || !used || !flag) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  RX_MESH_CLUSTERS(fn, n_clusters, n_vertices);
  RX_MESH_TRIANGLES(fn, n_triangles);
  if (!RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(cluster_of, 8) || !RX_MESH_ALIGNED(counts, 4) || !RX_MESH_ALIGNED(used, 4) || !RX_MESH_ALIGNED(flag, 4))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)n_clusters * 4, st) != hipSuccess || hipMemsetAsync(used, 0, (size_t)n_clusters * 4, st) != hipSuccess)
    RX_FAIL(RX_ELAUNCH, "%s: clearing the counts failed", fn);
  RX_MESH_LAUNCH(fn, md_remap_kernel, n_triangles, st, (const long long*)triangles, (long long)n_triangles, (long long)n_vertices,
            (const long long*)cluster_of, (long long)n_clusters, counts, used, flag);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_unique(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* cluster_of, int64_t n_clusters,
                                      const int64_t* entry_offsets, int32_t* cursor, int64_t capacity, int32_t* entries, int32_t* keep, void* stream) {
  const char* fn = "rx_mesh_cluster_unique";
  if (!triangles || !cluster_of || !entry_offsets) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!cursor || !keep || (capacity > 0 && !entries)) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  RX_MESH_CLUSTERS(fn, n_clusters, n_vertices);
  RX_MESH_TRIANGLES(fn, n_triangles);
  if (capacity < 0 || capacity > RX_MESH_MAX_TRIANGLES) RX_FAIL(RX_EINVAL, "%s: capacity %lld (0 .. (2^31 - 2) / 3 entries)", fn, (long long)capacity);
  if (!RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(cluster_of, 8) || !RX_MESH_ALIGNED(entry_offsets, 8) || !RX_MESH_ALIGNED(cursor, 4) || !RX_MESH_ALIGNED(entries, 4) ||
      !RX_MESH_ALIGNED(keep, 4))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(cursor, 0, (size_t)n_clusters * 4, st) != hipSuccess || hipMemsetAsync(keep, 0, (size_t)n_triangles * 4, st) != hipSuccess)
    RX_FAIL(RX_ELAUNCH, "%s: clearing the cursors failed", fn);
  if (capacity == 0) return RX_OK;      // no triangle survives
  RX_MESH_LAUNCH(fn, md_attach_kernel, n_triangles, st, (const long long*)triangles, (long long)n_triangles, (long long)n_vertices,
            (const long long*)cluster_of, (long long)n_clusters, (const long long*)entry_offsets, cursor, (long long)capacity, entries);
  RX_MESH_LAUNCH(fn, md_unique_kernel, n_clusters, st, (long long)n_clusters, (const long long*)entry_offsets, (long long)capacity, entries,
            (long long)n_triangles, keep);
  return RX_OK;
}

extern "C" int rx_mesh_cluster_emit(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* cluster_of, int64_t n_clusters,
                                    const int32_t* keep, const int64_t* keep_offsets, const int32_t* used, const int64_t* used_offsets,
                                    const float* representatives, int64_t vertex_capacity, float* out_vertices, int64_t triangle_capacity,
                                    int64_t* out_triangles, void* stream) {
  const char* fn = "rx_mesh_cluster_emit";
  if (!triangles || !cluster_of || !keep || !keep_offsets || !used || !used_offsets || !representatives) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if ((vertex_capacity > 0 && !out_vertices) || (triangle_capacity > 0 && !out_triangles)) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  RX_MESH_VERTICES(fn, n_vertices);
  RX_MESH_CLUSTERS(fn, n_clusters, n_vertices);
  RX_MESH_TRIANGLES(fn, n_triangles);
  if (vertex_capacity < 0 || triangle_capacity < 0) RX_FAIL(RX_EINVAL, "%s: negative capacity", fn);
  if (!RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(cluster_of, 8) || !RX_MESH_ALIGNED(keep, 4) || !RX_MESH_ALIGNED(keep_offsets, 8) || !RX_MESH_ALIGNED(used, 4) ||
      !RX_MESH_ALIGNED(used_offsets, 8) || !RX_MESH_ALIGNED(representatives, 4) || !RX_MESH_ALIGNED(out_vertices, 4) || !RX_MESH_ALIGNED(out_triangles, 8))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (triangle_capacity > 0)
    RX_MESH_LAUNCH(fn, md_emit_triangles_kernel, n_triangles, st, (const long long*)triangles, (long long)n_triangles, (long long)n_vertices,
              (const long long*)cluster_of, (long long)n_clusters, keep, (const long long*)keep_offsets, (const long long*)used_offsets,
              (long long)triangle_capacity, (long long*)out_triangles);
  if (vertex_capacity > 0)
    RX_MESH_LAUNCH(fn, md_emit_vertices_kernel, n_clusters, st, (long long)n_clusters, used, (const long long*)used_offsets, representatives,
              (long long)vertex_capacity, out_vertices);
  return RX_OK;
}
