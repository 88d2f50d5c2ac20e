// Polygon pool of the device rasterisers (mask targets: trainer.hip; validation canvases: engine.hip, val_ap.hip), host side: one
// contiguous block (one upload): int32 image_first[n_img + 1] | inst_first[n_inst + 1] | poly_off[n_poly] | poly_len[n_poly] | padding
// to 8 bytes | double xy[n_doubles].  poly_off counts doubles inside xy (the polygons are packed back to back in polygon order,
// whatever the caller's offsets were).
#pragma once
#include <string.h>

#include "common.h"

struct MtLayout {
  int n_img = 0, n_inst = 0, n_poly = 0;
  size_t n_doubles = 0, o_inst = 0, o_off = 0, o_len = 0, o_xy = 0, bytes = 0;
};
// offsets and size of a pool of these counts
inline void mt_layout(int n_img, int n_inst, int n_poly, size_t n_doubles, MtLayout* L) {
  L->n_img = n_img; L->n_inst = n_inst; L->n_poly = n_poly; L->n_doubles = n_doubles;
  L->o_inst = 4 * ((size_t)n_img + 1);
  L->o_off = L->o_inst + 4 * ((size_t)n_inst + 1);
  L->o_len = L->o_off + 4 * (size_t)n_poly;
  L->o_xy = (L->o_len + 4 * (size_t)n_poly + 7) & ~(size_t)7;
  L->bytes = L->o_xy + 8 * n_doubles;
}
inline int mt_measure(const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, int n_inst, int n_img, MtLayout* L) {
  RS_CHECK(inst_first && n_inst >= 0 && inst_first[0] == 0, RS_ERR_ARG, "polygons: inst_first must start at 0");
  for (int g = 0; g < n_inst; ++g) RS_CHECK(inst_first[g + 1] >= inst_first[g], RS_ERR_ARG, "polygons: inst_first decreases at instance %d", g);
  const int n_poly = inst_first[n_inst];
  RS_CHECK(n_poly == 0 || (polys && poly_off && poly_len), RS_ERR_ARG, "polygons: null table");
  size_t n_doubles = 0;
  for (int q = 0; q < n_poly; ++q) {
    RS_CHECK(poly_len[q] >= 2 && !(poly_len[q] & 1) && poly_off[q] >= 0, RS_ERR_ARG, "polygon %d: %d doubles at offset %lld", q, poly_len[q], (long long)poly_off[q]);
    n_doubles += (size_t)poly_len[q];
  }
  mt_layout(n_img, n_inst, n_poly, n_doubles, L);
  return RS_OK;
}
inline void mt_pack(uint8_t* dst, const MtLayout& L, const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first,
                    const int32_t* image_first) {
  memcpy(dst, image_first, 4 * ((size_t)L.n_img + 1));
  memcpy(dst + L.o_inst, inst_first, 4 * ((size_t)L.n_inst + 1));
  int32_t* off = (int32_t*)(dst + L.o_off);
  double* xy = (double*)(dst + L.o_xy);
  size_t at = 0;
  for (int q = 0; q < L.n_poly; ++q) {
    off[q] = (int32_t)at;
    memcpy(xy + at, polys + poly_off[q], 8 * (size_t)poly_len[q]);
    at += (size_t)poly_len[q];
  }
  if (L.n_poly) memcpy(dst + L.o_len, poly_len, 4 * (size_t)L.n_poly);
}
