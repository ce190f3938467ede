// tmatch_handle.hpp -- the payne_tmatch handle, shared by k_tmatch.hip (create, match, destroy) and k_tmatch_poly.hip (create_poly,
// match_poly).  payne_tmatch_create leaves max_poly = 0 and the poly workspace null: such a handle refuses payne_tmatch_match_poly.
#pragma once

struct payne_tmatch {
  int device = 0, max_stars = 0, max_templates = 0;
  double* part_c = nullptr;   // [chunks][N][topk]
  int* part_i = nullptr;
  int max_poly = 0;           // payne_tmatch_create_poly's; its workspace, per chunk of payne_tmatch_poly_chunk() templates:
  double* poly_c = nullptr;   // [chunks][N][topk]
  int* poly_i = nullptr;
  double* poly_coef = nullptr;   // [chunks][N][topk][P]
};
