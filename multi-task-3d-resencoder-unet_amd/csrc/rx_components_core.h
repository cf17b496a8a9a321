// rx_components_core.h -- the find / union / tile-merge logic of the connected-component pass (rx_components.hip), written so
// that it compiles for the host as well: csrc/tools/components_host_check.cpp runs exactly these functions serially, tile by
// tile, against a breadth-first search, under the address and undefined-behaviour sanitizers.
//
// A forest is an array of parents addressed through a small accessor `M`:
//     int  M::parent(int i)            the parent of node i (a root is its own parent); may return an OLDER parent of i
//     int  M::parent_min(int i, int p) parent(i) = min(parent(i), p), atomically; returns the parent it replaced
// The kernels give it LDS words (a tile's local forest) or the label volume itself (label = parent + 1, 0 = background) read
// with relaxed agent-scope loads; the host check gives it a plain array.
//
// Geometry: a tile is RX_CC_TZ x RX_CC_TY x RX_CC_TX voxels, RX_CC_TX = 64 = one wave along x; a tile row is (tz, ty) and its
// foreground is one 64-bit mask (the wave's ballot).  Local index l = (tz * RX_CC_TY + ty) * 64 + tx grows with the volume's
// linear index z*Y*X + y*X + x, so "the smaller index" means the same thing in a tile and in the volume.
#ifndef RX_COMPONENTS_CORE_H
#define RX_COMPONENTS_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define RX_CC_HD __host__ __device__ __forceinline__
#else
#define RX_CC_HD inline
#endif

#define RX_CC_TX 64
#define RX_CC_TY 8
#define RX_CC_TZ 8
#define RX_CC_ROWS (RX_CC_TZ * RX_CC_TY)
#define RX_CC_TILE (RX_CC_ROWS * RX_CC_TX)
#ifndef RX_CC_MAX_VOXELS
#define RX_CC_MAX_VOXELS 2147483646L      // 2^31 - 2: label = index + 1 stays an int32 (include/rxunet.h says the same)
#endif

// the largest number of non-zero offset components between neighbours: 6 -> 1 (faces), 18 -> 2 (+ edges), 26 -> 3 (+ corners); else 0
RX_CC_HD int cc_max_steps(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

// the first lane of the run of set bits that lane `lane` (whose bit is set) belongs to
RX_CC_HD int cc_run_start(uint64_t mask, int lane) {
  const uint64_t holes = ~mask & ((1ull << lane) - 1ull);      // the clear bits below the lane
  // the compiler builtin, the same expression in the kernel and in the host check (gcc and clang both have it)
  return holes == 0ull ? 0 : 64 - __builtin_clzll(holes);
}

template <class M>
RX_CC_HD int cc_find(M& m, int x) {
  // parent(i) <= i always (cc_union), so the walk strictly descends and ends at a node that is its own parent
  for (;;) {
    const int p = m.parent(x);
    if (p == x) return x;
    x = p;
  }
}

// find with path halving: every node passed is pointed at its grandparent -- by parent_min, so a parent only ever decreases and
// what it is replaced by is an ancestor, which keeps the node in its tree
template <class M>
RX_CC_HD int cc_find_halve(M& m, int x) {
  for (;;) {
    const int p = m.parent(x);
    if (p == x) return x;
    const int g = m.parent(p);
    if (g != p) m.parent_min(x, g);
    x = p;
  }
}

template <class M>
RX_CC_HD void cc_union(M& m, int a, int b) {
  // The standard lock-free union: find both roots, then parent_min the LARGER root's parent to the smaller; if the word no
  // longer held the larger root (another union got there first, or the "root" came from an older read) carry on from what it
  // did hold -- the word now holds the smaller of the two candidates, and the one that was displaced still has to be joined to
  // the other, which is what the next round does.  A larger root is only ever linked under a smaller one, so parent(i) <= i holds
  // at every moment: every find terminates, no cycle can form, and the minimum index of a component can never get a parent other
  // than itself.  When all unions are done each component is one tree, so its root is its minimum index whatever the arrival order.
  for (;;) {
    a = cc_find_halve(m, a);
    b = cc_find_halve(m, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }      // a is the larger root
    const int old = m.parent_min(a, b);
    if (old == a) return;      // a was a root and now hangs under b
    a = old;                   // lost: `old` (an ancestor-or-partner of a) and b are still to be joined
  }
}

RX_CC_HD bool cc_bit(uint64_t mask, int x) { return x >= 0 && x < 64 && ((mask >> x) & 1ull) != 0ull; }

// ---- inside a tile ---------------------------------------------------------------------------------------------------------------
// The x-runs of every row are already one tree each (every voxel seeded with its run start).  The foreground voxel (tz, ty, tx)
// joins its run to the runs it touches in the four tile rows that precede its own: (0,-1), (-1,-1), (-1,0), (-1,+1).  In such a
// row the neighbours at tx-1, tx, tx+1 lie in at most two runs.  If the one at tx is set it stands for all three, and the voxel
// leaves the union to its left neighbour when that one sees the same pair of runs; else the diagonal ones are taken, unless the
// voxel's own row neighbour on that side is set and so has the diagonal one straight below it.
template <class M>
RX_CC_HD void cc_tile_voxel(M& lds, const uint64_t* masks, int tz, int ty, int tx, int max_steps) {
  const int row = tz * RX_CC_TY + ty, self = row * RX_CC_TX + tx;
  const uint64_t own = masks[row];
  for (int k = 0; k < 4; ++k) {
    const int dz = k == 0 ? 0 : -1, dy = k == 0 ? -1 : k - 2;      // (0,-1) (-1,-1) (-1,0) (-1,+1)
    const int steps = (dz != 0) + (dy != 0);
    const int z2 = tz + dz, y2 = ty + dy;
    if (steps > max_steps || z2 < 0 || y2 < 0 || y2 >= RX_CC_TY) continue;
    const int row2 = z2 * RX_CC_TY + y2;
    const uint64_t other = masks[row2];
    if (cc_bit(other, tx)) {
      if (!(cc_bit(own, tx - 1) && cc_bit(other, tx - 1))) cc_union(lds, self, row2 * RX_CC_TX + tx);
    } else if (steps + 1 <= max_steps) {
      if (cc_bit(other, tx - 1) && !cc_bit(own, tx - 1)) cc_union(lds, self, row2 * RX_CC_TX + tx - 1);
      if (cc_bit(other, tx + 1) && !cc_bit(own, tx + 1)) cc_union(lds, self, row2 * RX_CC_TX + tx + 1);
    }
  }
}

// ---- across tile faces -------------------------------------------------------------------------------------------------------------
// Two neighbouring voxels in different tiles differ in their tile index along at least one axis; on that axis one of them lies on
// its tile's low face (coordinate a multiple of the tile extent) and the other one step below it.  So the low-face voxels of
// each axis, each looking at its nine neighbours one step down that axis, see every pair that crosses a tile face, edge or corner
// (some pairs twice, which a union does not mind).  `axis`: 0 = z, 1 = y, 2 = x.  The volume's accessor also answers M::label(i), 0 on
// background, and M::set_parent(i, p) for the flatten pass.  Along x a set middle neighbour stands for its two row neighbours, as inside a tile.
template <class M>
RX_CC_HD void cc_seam_voxel(M& vol, int axis, int z, int y, int x, int Z, int Y, int X, int max_steps) {
  const long XY = (long)Y * X;
  const int self = (int)(z * XY + (long)y * X + x);
  if (vol.label(self) == 0) return;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b) {
      // (a, b) run over the two axes other than `axis`, slower axis first; the step along `axis` is -1
      const int dz = axis == 0 ? -1 : a, dy = axis == 1 ? -1 : (axis == 0 ? a : b), dx = axis == 2 ? -1 : b;
      if ((dz != 0) + (dy != 0) + (dx != 0) > max_steps) continue;
      const int z2 = z + dz, y2 = y + dy, x2 = x + dx;
      if (z2 < 0 || z2 >= Z || y2 < 0 || y2 >= Y || x2 < 0 || x2 >= X) continue;      // never leaves the volume
      const int nb = (int)(z2 * XY + (long)y2 * X + x2);
      if (axis != 2 && dx != 0 && (dz != 0) + (dy != 0) <= max_steps && vol.label(nb - dx) != 0) continue;      // the middle one is set
      if (vol.label(nb) != 0) cc_union(vol, self, nb);
    }
}

// ---- flatten ---------------------------------------------------------------------------------------------------------------------
// label = root + 1.  Written over the parent word itself: root + 1 is "parent = root", so a walk that passes through a word
// that has already been flattened simply arrives sooner.
template <class M>
RX_CC_HD void cc_flatten_voxel(M& vol, int i) {
  if (vol.label(i) == 0) return;
  vol.set_parent(i, cc_find(vol, i));
}

#endif /* RX_COMPONENTS_CORE_H */
