// Device polygoniser: the mask -> polygon -> Ramer-Douglas-Peucker tail of the detector step (csrc/vectorize.cpp on the host,
// oracle/host_tail_oracle.py as its statement), one workgroup per instance, integer and LDS work only.  DESIGN.md 3.7 derives the
// formulation; tests/polygonize_ref.py states it in Python and is compared with the oracle on the CPU.
//
//   1 edges      every foreground pixel, row-major, emits its top (E), right (S), bottom (W), left (N) boundary edge; an edge is its
//                emission index t = 4 * (y * cw + x) + k, kept sorted (T).  Everything else about an edge is derived from t.
//   2 successor  static: at the head vertex the first of (d+1, d, d+3) mod 4 that exists.  A bijection on the edges; stored inverted (PRED)
//                together with "the direction changes here" (bit 15).
//   3 rings      key(e) = 2 * (index of the first-emitted edge at e's start vertex) + (e is the second one).  Pointer doubling over PRED
//                gives every edge its cycle's smallest key: the ring's start edge; rings are ordered by that key.
//   4 vertices   doubling again over PRED cut at the start edge counts the direction changes from the start edge to each edge: the
//                position of its vertex in the ring.  Rings are stored reversed (rasterio's direction), start vertex kept.
//   5 area       twice the shoelace area from the unit edges, integer atomics (wrap-around arithmetic is exact: |2A| < 2^31).
//   6 holes      probe point in doubled integers, crossing test over the exteriors' vertical edges, smallest area wins, first on a tie.
//   7 RDP        one wave per ring, explicit stack sized by the ring, integer argmax (first maximum), fp64 only in the comparison
//                with epsilon (-ffp-contract=off, as the host).
// Every loop bound is known before the loop starts; no float atomics; nothing crosses workgroups; the result is a function of the mask.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/rs_engine.h"
#include "common.h"
#include "polygonize.h"

namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_EPT = PG_EDGE_CAP / PG_THREADS;   // edges per thread in the doubling rounds (registers)
constexpr int PG_NIL = 0xFFFF;

// LDS layout (bytes).  The edge block is dead once the vertices are written; RDP's keep flags, stacks and the prefix of the flags reuse it.
constexpr int L_T = 0;                               // u32 [EDGE_CAP]  emission index
constexpr int L_VAL = L_T + 4 * PG_EDGE_CAP;         // u32 [EDGE_CAP]  hi: smallest key seen, lo: own key, later the vertex count
constexpr int L_PRED = L_VAL + 4 * PG_EDGE_CAP;      // u16 [EDGE_CAP]  predecessor | turn << 15
constexpr int L_NXT = L_PRED + 2 * PG_EDGE_CAP;      // u16 [EDGE_CAP]  doubling pointer
constexpr int L_EDGE_END = L_NXT + 2 * PG_EDGE_CAP;
constexpr int L_KEEP = 0;                            // u8  [VERTEX_CAP]
constexpr int L_STK = L_KEEP + PG_VERTEX_CAP;        // u32 [VERTEX_CAP]
constexpr int L_PK = L_STK + 4 * PG_VERTEX_CAP;      // u16 [VERTEX_CAP]
static_assert(L_PK + 2 * PG_VERTEX_CAP <= L_EDGE_END, "RDP scratch must fit in the edge block");
constexpr int L_VERT = L_EDGE_END;                   // u32 [VERTEX_CAP] x | y << 16, tile coordinates
constexpr int L_BM = L_VERT + 4 * PG_VERTEX_CAP;     // u32 [2 * EDGE_CAP / 32] start keys
constexpr int PG_BMW = 2 * PG_EDGE_CAP / 32;
constexpr int L_WP = L_BM + 4 * PG_BMW;              // i32 [BMW] start keys before each word
constexpr int L_TMP = L_WP + 4 * PG_BMW;             // i32 [THREADS] scan partials
constexpr int L_A2 = L_TMP + 4 * PG_THREADS;         // i32 [RING_CAP] twice the signed area
constexpr int L_R16 = L_A2 + 4 * PG_RING_CAP;        // u16 [11][RING_CAP] ring tables
constexpr int PG_LDS = L_R16 + 11 * 2 * PG_RING_CAP;
static_assert(PG_BMW == PG_THREADS, "one bitmap word per thread");
static_assert(PG_EDGE_CAP <= 0x7FFF && PG_VERTEX_CAP + PG_RING_CAP <= 0xFFFF, "16-bit indices");
static_assert(PG_LDS <= 160 * 1024, "LDS of one CU");

struct Img {
  const uint8_t* base;
  int stride, cw, rows;
};

__device__ inline int pix(const Img& g, int x, int y) {
  if ((unsigned)x >= (unsigned)g.cw || (unsigned)y >= (unsigned)g.rows) return 0;
  return (g.base[(long long)y * g.stride + (x >> 3)] >> (x & 7)) & 1;
}
// eight pixels of row y starting at pixel 8 * bx, zero outside the image
__device__ inline unsigned rowbyte(const Img& g, int bx, int y) {
  if ((unsigned)y >= (unsigned)g.rows || bx < 0 || bx * 8 >= g.cw) return 0u;
  unsigned v = g.base[(long long)y * g.stride + bx];
  const int rem = g.cw - bx * 8;
  if (rem < 8) v &= (1u << rem) - 1u;
  return v;
}
__device__ inline void edge_masks(const Img& g, int bx, int y, unsigned m[4]) {
  const unsigned f = rowbyte(g, bx, y);
  if (!f) { m[0] = m[1] = m[2] = m[3] = 0u; return; }
  const unsigned up = rowbyte(g, bx, y - 1), dn = rowbyte(g, bx, y + 1);
  const unsigned l = rowbyte(g, bx - 1, y) >> 7, r = rowbyte(g, bx + 1, y) & 1u;
  m[0] = f & ~up;                               // top    -> E
  m[1] = f & ~((f >> 1) | (r << 7));            // right  -> S
  m[2] = f & ~dn;                               // bottom -> W
  m[3] = f & ~(((f << 1) | l) & 0xFFu);         // left   -> N
}
// outgoing directions of vertex (x, y): bit d set = an edge leaves in direction d (0 E, 1 S, 2 W, 3 N), foreground on its right
__device__ inline unsigned vertex_dirs(const Img& g, int x, int y) {
  const int a = pix(g, x - 1, y - 1), b = pix(g, x, y - 1), c = pix(g, x - 1, y), d = pix(g, x, y);
  return (unsigned)(d & ~b & 1) | ((unsigned)(c & ~d & 1) << 1) | ((unsigned)(a & ~c & 1) << 2) | ((unsigned)(b & ~a & 1) << 3);
}
// emission index of the edge that leaves vertex (x, y) in direction d
__device__ inline int edge_t(int cw, int x, int y, int d) {
  switch (d) {
    case 0: return 4 * (y * cw + x);
    case 1: return 4 * (y * cw + x - 1) + 1;
    case 2: return 4 * ((y - 1) * cw + x - 1) + 2;
    default: return 4 * ((y - 1) * cw + x) + 3;
  }
}
__device__ inline void edge_decode(int cw, int t, int& vx, int& vy, int& d) {
  d = t & 3;
  const int p = t >> 2;
  const int py = p / cw, px = p - py * cw;
  vx = px + (d == 1 || d == 2);
  vy = py + (d >= 2);
}
// index of t in the sorted T[0, E); t is always present, the clamp only keeps a wrong input inside the array
__device__ inline int find_edge(const unsigned* T, int E, unsigned t) {
  int lo = 0, hi = E - 1;
  while (lo < hi) {                               // at most ceil(log2 E) rounds
    const int mid = (lo + hi) >> 1;
    if (T[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// exclusive scan in place over a[0, n), n <= a few thousand; returns the sum.  Called by the whole workgroup.
template <typename T>
__device__ int block_exscan(T* a, int n, int* tmp) {
  const int tid = threadIdx.x;
  const int per = (n + PG_THREADS - 1) / PG_THREADS;
  const int b = tid * per;
  const int e = b + per < n ? b + per : n;
  int s = 0;
  for (int i = b; i < e; ++i) s += (int)a[i];
  tmp[tid] = s;
  __syncthreads();
  for (int off = 1; off < PG_THREADS; off <<= 1) {
    const int v = tid >= off ? tmp[tid - off] : 0;
    __syncthreads();
    tmp[tid] += v;
    __syncthreads();
  }
  int run = tmp[tid] - s;
  const int total = tmp[PG_THREADS - 1];
  for (int i = b; i < e; ++i) { const int v = (int)a[i]; a[i] = (T)run; run += v; }
  __syncthreads();
  return total;
}

__device__ inline int ceil_log2(int n) {
  int r = 0;
  while ((1 << r) < n) ++r;
  return r;
}

__global__ __launch_bounds__(PG_THREADS) void polygonize_trace_kernel(const PolyParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* T = (unsigned*)(smem + L_T);
  unsigned* VAL = (unsigned*)(smem + L_VAL);
  uint16_t* PRED = (uint16_t*)(smem + L_PRED);
  uint16_t* NXT = (uint16_t*)(smem + L_NXT);
  uint8_t* KEEP = (uint8_t*)(smem + L_KEEP);
  unsigned* STK = (unsigned*)(smem + L_STK);
  uint16_t* PK = (uint16_t*)(smem + L_PK);
  unsigned* VERT = (unsigned*)(smem + L_VERT);
  unsigned* BM = (unsigned*)(smem + L_BM);
  int* WP = (int*)(smem + L_WP);
  int* tmp = (int*)(smem + L_TMP);
  int* A2 = (int*)(smem + L_A2);
  uint16_t* R16 = (uint16_t*)(smem + L_R16);
  uint16_t* R_LEN = R16;                          // closed length before simplification
  uint16_t* R_OFF = R16 + PG_RING_CAP;            // first vertex in VERT
  uint16_t* R_OWN = R16 + 2 * PG_RING_CAP;        // ring index of the exterior that owns the ring (itself for an exterior), NIL = none
  uint16_t* R_K = R16 + 3 * PG_RING_CAP;          // a hole's rank among its owner's holes
  uint16_t* R_CNT = R16 + 4 * PG_RING_CAP;        // exterior: rings of its polygon, else 0
  uint16_t* R_BASE = R16 + 5 * PG_RING_CAP;       // exterior: first output ring of its polygon
  uint16_t* R_EORD = R16 + 6 * PG_RING_CAP;       // exteriors before this ring
  uint16_t* R_POS = R16 + 7 * PG_RING_CAP;        // output position of the ring, NIL = none
  uint16_t* R_ORD = R16 + 8 * PG_RING_CAP;        // ring at an output position
  uint16_t* R_OLEN = R16 + 9 * PG_RING_CAP;       // length after simplification
  uint16_t* R_OOFF = R16 + 10 * PG_RING_CAP;      // per output position: first output vertex

  const int inst = blockIdx.x;
  const int tid = threadIdx.x;
  int* hdr = p.s_hdr + (long long)inst * 4;
  auto finish = [&](int flag, int np, int nr, int nv) {
    if (tid == 0) { hdr[0] = flag; hdr[1] = np; hdr[2] = nr; hdr[3] = nv; }
  };
  if (p.det_count) {
    const int i = inst / p.D, d = inst - i * p.D;
    if (d >= p.det_count[i]) { finish(0, 0, 0, 0); return; }
  }
  int x0b = 0, oy = 0, wbytes = p.Wb, rows = p.h;
  if (p.rects) {
    const int* r = p.rects + (long long)inst * 4;
    x0b = r[0]; oy = r[1]; wbytes = r[2]; rows = r[3];
    if (x0b < 0 || oy < 0 || wbytes < 0 || rows < 0 || x0b + wbytes > p.Wb || oy + rows > p.h) { finish(1, 0, 0, 0); return; }
  }
  if (wbytes <= 0 || rows <= 0) { finish(0, 0, 0, 0); return; }
  const int ox = x0b * 8;
  Img g;
  g.base = p.masks + ((long long)inst * p.h + oy) * p.Wb + x0b;
  g.stride = p.Wb;
  g.cw = ox + wbytes * 8 > p.w ? p.w - ox : wbytes * 8;
  g.rows = rows;
  const int cw = g.cw;

  // ---- 1: edges, in emission order (each thread a contiguous run of mask bytes: count, scan, write)
  const int items = wbytes * rows;
  const int per = (items + PG_THREADS - 1) / PG_THREADS;
  const int ib = tid * per;
  const int ie = ib + per < items ? ib + per : items;
  int mine = 0;
  for (int it = ib; it < ie; ++it) {
    const int y = it / wbytes, bx = it - y * wbytes;
    unsigned m[4];
    edge_masks(g, bx, y, m);
    mine += __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
  }
  tmp[tid] = mine;
  __syncthreads();
  for (int off = 1; off < PG_THREADS; off <<= 1) {
    const int v = tid >= off ? tmp[tid - off] : 0;
    __syncthreads();
    tmp[tid] += v;
    __syncthreads();
  }
  const int E = tmp[PG_THREADS - 1];
  int at = tmp[tid] - mine;
  __syncthreads();
  if (E == 0) { finish(0, 0, 0, 0); return; }
  if (E > p.edge_cap) { finish(1, 0, 0, 0); return; }
  for (int it = ib; it < ie; ++it) {
    const int y = it / wbytes, bx = it - y * wbytes;
    unsigned m[4];
    edge_masks(g, bx, y, m);
    unsigned any = m[0] | m[1] | m[2] | m[3];
    while (any) {                                  // at most 8 rounds
      const int b = __ffs(any) - 1;
      any &= any - 1;
      const int t0 = 4 * (y * cw + bx * 8 + b);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((m[k] >> b) & 1u) { if (at < E) T[at] = (unsigned)(t0 + k); ++at; }
    }
  }
  __syncthreads();

  // ---- 2, 3: successor (stored as predecessor + turn flag) and key
  for (int e = tid; e < E; e += PG_THREADS) PRED[e] = (uint16_t)e;      // overwritten below: the successor is a bijection
  __syncthreads();
  for (int e = tid; e < E; e += PG_THREADS) {
    const int t = (int)T[e];
    int vx, vy, d;
    edge_decode(cw, t, vx, vy, d);
    unsigned key = 2u * (unsigned)e;
    const unsigned other = vertex_dirs(g, vx, vy) & ~(1u << d);
    if (other) {
      const int to = edge_t(cw, vx, vy, __ffs(other) - 1);
      if (to < t) key = 2u * (unsigned)find_edge(T, E, (unsigned)to) + 1u;
    }
    VAL[e] = key | (key << 16);
    const int nx = vx + (d == 0) - (d == 2), ny = vy + (d == 1) - (d == 3);
    const unsigned hn = vertex_dirs(g, nx, ny);
    int c = (d + 1) & 3;
    if (!((hn >> c) & 1u)) c = d;
    if (!((hn >> c) & 1u)) c = (d + 3) & 3;
    const int sidx = find_edge(T, E, (unsigned)edge_t(cw, nx, ny, c));
    PRED[sidx] = (uint16_t)(e | ((c != d) << 15));
  }
  __syncthreads();
  const int rounds = ceil_log2(E);
  for (int e = tid; e < E; e += PG_THREADS) NXT[e] = PRED[e] & 0x7FFF;
  __syncthreads();
  for (int r = 0; r < rounds; ++r) {
    unsigned mv[PG_EPT];
    uint16_t nn[PG_EPT];
#pragma unroll
    for (int j = 0; j < PG_EPT; ++j) {
      const int e = tid + j * PG_THREADS;
      if (e < E) { const int n = NXT[e]; nn[j] = NXT[n]; mv[j] = VAL[n] >> 16; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PG_EPT; ++j) {
      const int e = tid + j * PG_THREADS;
      if (e < E) {
        const unsigned cur = VAL[e];
        const unsigned mn = (cur >> 16) < mv[j] ? (cur >> 16) : mv[j];
        VAL[e] = (cur & 0xFFFFu) | (mn << 16);
        NXT[e] = nn[j];
      }
    }
    __syncthreads();
  }
  // ring index = number of start keys below the ring's
  BM[tid] = 0u;
  __syncthreads();
  for (int e = tid; e < E; e += PG_THREADS) {
    const unsigned v = VAL[e];
    if ((v >> 16) == (v & 0xFFFFu)) atomicOr(&BM[(v & 0xFFFFu) >> 5], 1u << (v & 31u));
  }
  __syncthreads();
  WP[tid] = __popc(BM[tid]);
  __syncthreads();
  const int R = block_exscan(WP, PG_BMW, tmp);
  if (R > PG_RING_CAP) { finish(1, 0, 0, 0); return; }
  auto ring_of = [&](unsigned key) { return WP[key >> 5] + __popc(BM[key >> 5] & ((1u << (key & 31u)) - 1u)); };

  // ---- 4: position of every vertex in its ring
  for (int e = tid; e < E; e += PG_THREADS) {
    const unsigned v = VAL[e];
    const unsigned pr = PRED[e];
    const bool start = (v >> 16) == (v & 0xFFFFu);
    if (start) R_ORD[ring_of(v >> 16)] = (uint16_t)e;          // the ring's start edge (R_ORD is free until step 6)
    NXT[e] = start ? (uint16_t)PG_NIL : (uint16_t)(pr & 0x7FFFu);
    VAL[e] = (v & 0xFFFF0000u) | (pr >> 15);
  }
  __syncthreads();
  for (int r = 0; r < rounds; ++r) {
    unsigned cv[PG_EPT];
    uint16_t nn[PG_EPT];
#pragma unroll
    for (int j = 0; j < PG_EPT; ++j) {
      const int e = tid + j * PG_THREADS;
      cv[j] = 0u; nn[j] = (uint16_t)PG_NIL;
      if (e < E) { const int n = NXT[e]; if (n != PG_NIL) { cv[j] = VAL[n] & 0xFFFFu; nn[j] = NXT[n]; } }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PG_EPT; ++j) {
      const int e = tid + j * PG_THREADS;
      if (e < E) { VAL[e] += cv[j]; NXT[e] = nn[j]; }
    }
    __syncthreads();
  }
  // ring length = direction changes of the whole cycle (the count at the start edge's predecessor) + the closing vertex
  for (int r = tid; r < R; r += PG_THREADS) {
    const int last = PRED[R_ORD[r]] & 0x7FFF;
    R_LEN[r] = (uint16_t)((VAL[last] & 0xFFFFu) + 1u);
    A2[r] = 0;
  }
  __syncthreads();
  for (int r = tid; r < R; r += PG_THREADS) R_OFF[r] = R_LEN[r];
  __syncthreads();
  const int V = block_exscan(R_OFF, R, tmp);
  if (V > p.vertex_cap) { finish(1, 0, 0, 0); return; }
  for (int e = tid; e < E; e += PG_THREADS) {
    const unsigned v = VAL[e];
    const int rid = ring_of(v >> 16);
    int vx, vy, d;
    edge_decode(cw, (int)T[e], vx, vy, d);
    vx += ox; vy += oy;
    // ---- 5: twice the area: sum of x0 * y1 - x1 * y0 over unit edges
    atomicAdd(&A2[rid], d == 0 ? -vy : d == 1 ? vx : d == 2 ? vy : -vx);
    if (PRED[e] >> 15) {
      const int pos = (int)(v & 0xFFFFu) - 1;
      const int m = R_LEN[rid] - 1, off = R_OFF[rid];
      const unsigned xy = (unsigned)vx | ((unsigned)vy << 16);
      if (pos == 0) { VERT[off] = xy; VERT[off + m] = xy; }
      else VERT[off + m - pos] = xy;               // reversed, start vertex kept
    }
  }
  __syncthreads();

  // ---- 6: holes -> exteriors
  for (int r = tid; r < R; r += PG_THREADS) {
    int own = r;
    if (A2[r] < 0) {
      const int off = R_OFF[r], L = R_LEN[r];
      const unsigned v0 = VERT[off], v1 = VERT[off + L - 2];          // first two vertices in traced order
      const int hx0 = v0 & 0xFFFF, hy0 = v0 >> 16, hx1 = v1 & 0xFFFF, hy1 = v1 >> 16;
      const int dx = hx1 - hx0, dy = hy1 - hy0;
      const int px2 = hx0 + hx1 + (dy > 0) - (dy < 0), py2 = hy0 + hy1 - (dx > 0) + (dx < 0);
      own = PG_NIL;
      int best_area = 0;
      for (int x = 0; x < R; ++x) {
        if (A2[x] <= 0) continue;
        const int xo = R_OFF[x], xl = R_LEN[x];
        int inside = 0;
        unsigned a = VERT[xo];
        for (int i = 1; i < xl; ++i) {
          const unsigned b = VERT[xo + i];
          const int ya = 2 * (int)(a >> 16), yb = 2 * (int)(b >> 16);
          if ((ya > py2) != (yb > py2) && 2 * (int)(a & 0xFFFF) > px2) inside ^= 1;
          a = b;
        }
        if (inside && (own == PG_NIL || A2[x] < best_area)) { own = x; best_area = A2[x]; }
      }
    }
    R_OWN[r] = (uint16_t)own;
  }
  __syncthreads();
  for (int r = tid; r < R; r += PG_THREADS) {
    const bool ext = A2[r] > 0;
    int k = 0;
    if (ext) { for (int q = 0; q < R; ++q) k += (A2[q] < 0 && R_OWN[q] == r); }
    else { const int own = R_OWN[r]; for (int q = 0; q < r; ++q) k += (A2[q] < 0 && R_OWN[q] == own); }
    R_K[r] = (uint16_t)k;
    R_CNT[r] = ext ? (uint16_t)(1 + k) : (uint16_t)0;
    R_BASE[r] = R_CNT[r];
    R_EORD[r] = ext ? 1 : 0;
  }
  __syncthreads();
  const int Rout = block_exscan(R_BASE, R, tmp);
  const int P = block_exscan(R_EORD, R, tmp);
  for (int r = tid; r < R; r += PG_THREADS) {
    int pos = PG_NIL;
    if (A2[r] > 0) pos = R_BASE[r];
    else if (R_OWN[r] != PG_NIL) pos = R_BASE[R_OWN[r]] + 1 + R_K[r];
    R_POS[r] = (uint16_t)pos;
    if (pos != PG_NIL) R_ORD[pos] = (uint16_t)r;
  }
  // ---- 7: Ramer-Douglas-Peucker (the edge block is dead from here on)
  const bool simplify = p.eps > 0;
  for (int i = tid; i < V; i += PG_THREADS) KEEP[i] = simplify ? 0 : 1;
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  if (simplify) {
    for (int r = wave; r < R; r += PG_THREADS / 64) {
      const int off = R_OFF[r], n = R_LEN[r];
      KEEP[off] = 1; KEEP[off + n - 1] = 1;
      int sp = 0;
      STK[off + sp++] = (unsigned)(n - 1) << 16;
      // every value below is the same in all lanes of the wave; every lane writes the stack and the flags, so each lane reads what it wrote
      for (int guard = 0; guard < 2 * n && sp > 0; ++guard) {
        const unsigned seg = STK[off + --sp];
        const int i0 = seg & 0xFFFF, i1 = seg >> 16;
        if (i1 <= i0 + 1) continue;
        const unsigned a = VERT[off + i0], b = VERT[off + i1];
        const int ax = a & 0xFFFF, ay = a >> 16;
        const int sx = (int)(b & 0xFFFF) - ax, sy = (int)(b >> 16) - ay;
        const bool degenerate = sx == 0 && sy == 0;
        int best = -1, bk = 0x7FFFFFFF;
        for (int k = i0 + 1 + lane; k < i1; k += 64) {
          const unsigned q = VERT[off + k];
          const int qx = (int)(q & 0xFFFF) - ax, qy = (int)(q >> 16) - ay;
          int val = degenerate ? qx * qx + qy * qy : sx * qy - sy * qx;
          val = val < 0 ? -val : val;
          if (val > best) { best = val; bk = k; }
        }
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
          const int ov = __shfl_xor(best, sft, 64), ok = __shfl_xor(bk, sft, 64);
          if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
        }
        const double dist = degenerate ? sqrt((double)best) : (double)best / sqrt((double)(sx * sx + sy * sy));
        if (dist > p.eps && sp + 2 <= n) {
          KEEP[off + bk] = 1;
          STK[off + sp++] = (unsigned)i0 | ((unsigned)bk << 16);
          STK[off + sp++] = (unsigned)bk | ((unsigned)i1 << 16);
        }
      }
    }
  }
  __syncthreads();
  for (int r = wave; r < R; r += PG_THREADS / 64) {
    const int off = R_OFF[r], n = R_LEN[r];
    int cnt = 0;
    for (int k = lane; k < n; k += 64) cnt += KEEP[off + k];
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) cnt += __shfl_xor(cnt, sft, 64);
    if (cnt < 4) {                                   // a ring that would drop below 4 points keeps its vertices
      for (int k = lane; k < n; k += 64) KEEP[off + k] = 1;
      cnt = n;
    }
    if (lane == 0) R_OLEN[r] = (uint16_t)cnt;
  }
  __syncthreads();
  // ---- output tables of the instance
  for (int i = tid; i < V; i += PG_THREADS) PK[i] = KEEP[i];
  for (int j = tid; j < Rout; j += PG_THREADS) R_OOFF[j] = R_OLEN[R_ORD[j]];
  __syncthreads();
  block_exscan(PK, V, tmp);
  const int Vout = block_exscan(R_OOFF, Rout, tmp);
  uint16_t* o_prc = p.s_prc + (long long)inst * PG_RING_CAP;
  uint16_t* o_rlen = p.s_rlen + (long long)inst * PG_RING_CAP;
  unsigned* o_xy = p.s_xy + (long long)inst * PG_VERTEX_CAP;
  for (int r = tid; r < R; r += PG_THREADS) {
    if (A2[r] > 0) o_prc[R_EORD[r]] = R_CNT[r];
    if (R_POS[r] < PG_RING_CAP) o_rlen[R_POS[r]] = R_OLEN[r];
  }
  for (int r = wave; r < R; r += PG_THREADS / 64) {
    if (R_POS[r] == PG_NIL) continue;
    const int off = R_OFF[r], n = R_LEN[r], base = R_OOFF[R_POS[r]] - PK[off];
    for (int k = lane; k < n; k += 64)
      if (KEEP[off + k]) { const int at2 = base + PK[off + k]; if (at2 >= 0 && at2 < PG_VERTEX_CAP) o_xy[at2] = VERT[off + k]; }
  }
  finish(0, P, Rout, Vout);
}

// offsets of every instance's rows in the compacted tables (one workgroup; instances are a few thousand at the most)
__global__ __launch_bounds__(PG_THREADS) void polygonize_plan_kernel(const PolyParams p) {
  __shared__ int part[3][PG_THREADS];
  __shared__ int nflag[PG_THREADS];
  const int tid = threadIdx.x;
  const int per = (p.instances + PG_THREADS - 1) / PG_THREADS;
  const int b = tid * per;
  const int e = b + per < p.instances ? b + per : p.instances;
  int s[3] = {0, 0, 0}, f = 0;
  for (int i = b; i < e; ++i) {
    const int* h = p.s_hdr + (long long)i * 4;
    f += h[0] != 0;
    for (int k = 0; k < 3; ++k) s[k] += h[1 + k];
  }
  for (int k = 0; k < 3; ++k) part[k][tid] = s[k];
  nflag[tid] = f;
  __syncthreads();
  for (int off = 1; off < PG_THREADS; off <<= 1) {
    int v[3] = {0, 0, 0}, vf = 0;
    if (tid >= off) { for (int k = 0; k < 3; ++k) v[k] = part[k][tid - off]; vf = nflag[tid - off]; }
    __syncthreads();
    for (int k = 0; k < 3; ++k) part[k][tid] += v[k];
    nflag[tid] += vf;
    __syncthreads();
  }
  int run[3];
  for (int k = 0; k < 3; ++k) run[k] = part[k][tid] - s[k];
  for (int i = b; i < e; ++i) {
    const int* h = p.s_hdr + (long long)i * 4;
    int* o = p.header + (long long)i * PG_HDR;
    o[0] = h[0]; o[1] = h[1]; o[2] = h[2]; o[3] = h[3];
    o[4] = run[0]; o[5] = run[1]; o[6] = run[2]; o[7] = 0;
    for (int k = 0; k < 3; ++k) run[k] += h[1 + k];
  }
  if (tid == PG_THREADS - 1) {
    p.totals[0] = part[0][tid]; p.totals[1] = part[1][tid]; p.totals[2] = part[2][tid]; p.totals[3] = nflag[tid];
  }
}

__global__ __launch_bounds__(PG_THREADS) void polygonize_compact_kernel(const PolyParams p) {
  const int inst = blockIdx.x;
  const int* h = p.header + (long long)inst * PG_HDR;
  const int np = h[1], nr = h[2], nv = h[3];
  const uint16_t* prc = p.s_prc + (long long)inst * PG_RING_CAP;
  const uint16_t* rlen = p.s_rlen + (long long)inst * PG_RING_CAP;
  const unsigned* xy = p.s_xy + (long long)inst * PG_VERTEX_CAP;
  for (int i = threadIdx.x; i < np && i < PG_RING_CAP; i += PG_THREADS) p.poly_ring_count[h[4] + i] = prc[i];
  for (int i = threadIdx.x; i < nr && i < PG_RING_CAP; i += PG_THREADS) p.ring_len[h[5] + i] = rlen[i];
  for (int i = threadIdx.x; i < nv && i < PG_VERTEX_CAP; i += PG_THREADS) p.xy[h[6] + i] = xy[i];
}

}  // namespace

size_t polygonize_scratch_bytes(int instances, size_t* hdr, size_t* prc, size_t* rlen, size_t* xy) {
  const size_t a = (size_t)instances * 16, b = (size_t)instances * PG_RING_CAP * 2, c = b, d = (size_t)instances * PG_VERTEX_CAP * 4;
  if (hdr) *hdr = a;
  if (prc) *prc = b;
  if (rlen) *rlen = c;
  if (xy) *xy = d;
  return a + b + c + d;
}

int launch_polygonize(const PolyParams& p, hipStream_t s) {
  RS_CHECK(p.masks && p.instances > 0 && p.D > 0 && p.s_hdr && p.s_prc && p.s_rlen && p.s_xy && p.header && p.poly_ring_count && p.ring_len && p.xy &&
               p.totals, RS_ERR_ARG, "polygonize: bad argument");
  RS_CHECK(p.h > 0 && p.w > 0 && p.h <= PG_MAX_SIDE && p.w <= PG_MAX_SIDE && p.Wb == (p.w + 7) / 8, RS_ERR_UNSUPPORTED,
           "polygonize: canvas %d x %d outside [1, %d]", p.h, p.w, PG_MAX_SIDE);
  RS_CHECK(p.edge_cap >= 1 && p.edge_cap <= PG_EDGE_CAP && p.vertex_cap >= 1 && p.vertex_cap <= PG_VERTEX_CAP, RS_ERR_ARG,
           "polygonize: caps %d / %d outside [1, %d] / [1, %d]", p.edge_cap, p.vertex_cap, PG_EDGE_CAP, PG_VERTEX_CAP);
  static bool attr = false;
  if (!attr) {
    RS_HIP(hipFuncSetAttribute((const void*)polygonize_trace_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PG_LDS));
    attr = true;
  }
  hipLaunchKernelGGL(polygonize_trace_kernel, dim3(p.instances), dim3(PG_THREADS), PG_LDS, s, p);
  hipLaunchKernelGGL(polygonize_plan_kernel, dim3(1), dim3(PG_THREADS), 0, s, p);
  hipLaunchKernelGGL(polygonize_compact_kernel, dim3(p.instances), dim3(PG_THREADS), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

extern "C" {

void rs_polygonize_caps(int* edge_cap, int* vertex_cap, int* ring_cap, int* max_side) {
  if (edge_cap) *edge_cap = PG_EDGE_CAP;
  if (vertex_cap) *vertex_cap = PG_VERTEX_CAP;
  if (ring_cap) *ring_cap = PG_RING_CAP;
  if (max_side) *max_side = PG_MAX_SIDE;
}

// the two stand-alone forms: scratch of the call's own, one launch_polygonize, wait
static int op_polygonize(const char* who, const uint8_t* masks_dev, int n, int slots, const int32_t* det_count_dev, const int32_t* rects_dev, int h, int w,
                         double rdp_epsilon, int edge_cap, int vertex_cap, int32_t* header_dev, int32_t* poly_ring_count_dev, int32_t* ring_len_dev,
                         int16_t* xy_dev, int32_t* totals_dev, void* stream) {
  RS_CHECK(masks_dev && n > 0 && slots > 0 && header_dev && poly_ring_count_dev && ring_len_dev && xy_dev && totals_dev, RS_ERR_ARG, "%s: bad argument", who);
  RS_CHECK(edge_cap >= 0 && vertex_cap >= 0, RS_ERR_ARG, "%s: negative cap", who);
  hipStream_t s = (hipStream_t)stream;
  size_t b_hdr, b_prc, b_rlen, b_xy;
  const size_t total = polygonize_scratch_bytes(n, &b_hdr, &b_prc, &b_rlen, &b_xy);
  char* scratch = nullptr;
  RS_HIP(hipMalloc((void**)&scratch, total));
  PolyParams p;
  memset(&p, 0, sizeof p);
  p.masks = masks_dev; p.rects = rects_dev; p.det_count = det_count_dev; p.instances = n; p.D = slots; p.h = h; p.w = w; p.Wb = (w + 7) / 8; p.eps = rdp_epsilon;
  p.edge_cap = edge_cap ? edge_cap : PG_EDGE_CAP; p.vertex_cap = vertex_cap ? vertex_cap : PG_VERTEX_CAP;
  p.s_hdr = (int*)scratch; p.s_prc = (uint16_t*)(scratch + b_hdr); p.s_rlen = (uint16_t*)(scratch + b_hdr + b_prc);
  p.s_xy = (uint32_t*)(scratch + b_hdr + b_prc + b_rlen);
  p.header = header_dev; p.poly_ring_count = poly_ring_count_dev; p.ring_len = ring_len_dev; p.xy = (uint32_t*)xy_dev; p.totals = totals_dev;
  int rc = launch_polygonize(p, s);
  const hipError_t he = hipStreamSynchronize(s);
  (void)hipFree(scratch);
  if (rc) return rc;
  RS_HIP(he);
  return RS_OK;
}

int rs_op_polygonize(const uint8_t* masks_dev, int n, int h, int w, double rdp_epsilon, int edge_cap, int vertex_cap, int32_t* header_dev,
                     int32_t* poly_ring_count_dev, int32_t* ring_len_dev, int16_t* xy_dev, int32_t* totals_dev, void* stream) {
  return op_polygonize("rs_op_polygonize", masks_dev, n, 1, nullptr, nullptr, h, w, rdp_epsilon, edge_cap, vertex_cap, header_dev, poly_ring_count_dev,
                       ring_len_dev, xy_dev, totals_dev, stream);
}

int rs_op_polygonize_crops(const uint8_t* masks_dev, int tiles, int slots, const int32_t* det_count_dev, const int32_t* rects_dev, int h, int w,
                           double rdp_epsilon, int edge_cap, int vertex_cap, int32_t* header_dev, int32_t* poly_ring_count_dev, int32_t* ring_len_dev,
                           int16_t* xy_dev, int32_t* totals_dev, void* stream) {
  RS_CHECK(tiles > 0 && slots > 0 && (long long)tiles * slots <= 0x7FFFFFFF, RS_ERR_ARG, "rs_op_polygonize_crops: %d tiles of %d slots", tiles, slots);
  return op_polygonize("rs_op_polygonize_crops", masks_dev, tiles * slots, slots, det_count_dev, rects_dev, h, w, rdp_epsilon, edge_cap, vertex_cap, header_dev,
                       poly_ring_count_dev, ring_len_dev, xy_dev, totals_dev, stream);
}

}  // extern "C"
