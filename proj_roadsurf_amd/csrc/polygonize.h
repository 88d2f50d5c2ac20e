// Device polygoniser (csrc/polygonize.hip): bit-packed instance masks -> polygons along pixel edges -> Ramer-Douglas-Peucker,
// vertex for vertex what csrc/vectorize.cpp computes on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Per-instance capacities of the LDS working set (one workgroup per instance).  An instance that needs more is flagged and left to the host.
constexpr int PG_EDGE_CAP = 4096;     // directed unit edges
constexpr int PG_VERTEX_CAP = 4096;   // ring vertices before simplification, closing vertices included
constexpr int PG_RING_CAP = 512;      // rings (and polygons)
constexpr int PG_MAX_SIDE = 1024;     // canvas height / width: 2 * side^2 < 2^22 keeps the integer RDP argmax equal to numpy's
constexpr int PG_HDR = 8;             // int32 per instance: flag, polygons, rings, vertices, first polygon, first ring, first vertex, 0

struct PolyParams {
  const uint8_t* masks;     // [instances][h][Wb] bit-packed canvases
  const int* rects;         // [instances][4] first byte column, first row, bytes per row, rows (rs_mask_crops.rects); null = whole canvas
  const int* det_count;     // [instances / D] valid slots per tile; null = every instance is valid
  int instances, D, h, w, Wb;
  double eps;               // <= 0: no simplification
  int edge_cap, vertex_cap; // <= PG_EDGE_CAP / PG_VERTEX_CAP
  // per-instance scratch, fixed strides
  int* s_hdr;               // [instances][4] flag, polygons, rings, vertices
  uint16_t* s_prc;          // [instances][PG_RING_CAP] rings per polygon
  uint16_t* s_rlen;         // [instances][PG_RING_CAP] vertices per ring
  uint32_t* s_xy;           // [instances][PG_VERTEX_CAP] x | y << 16
  // compacted tables
  int* header;              // [instances][PG_HDR]
  int* poly_ring_count;     // [total polygons]
  int* ring_len;            // [total rings]
  uint32_t* xy;             // [total vertices] int16 x, int16 y in tile coordinates
  int* totals;              // [4] polygons, rings, vertices, flagged instances
};

size_t polygonize_scratch_bytes(int instances, size_t* hdr, size_t* prc, size_t* rlen, size_t* xy);
int launch_polygonize(const PolyParams& p, hipStream_t s);
