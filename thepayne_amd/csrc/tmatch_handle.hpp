// tmatch_handle.hpp -- the payne_tmatch handle, shared by k_tmatch.hip (create, match, destroy), k_tmatch_poly.hip (create_poly,
// match_poly) and k_tmatch_pair.hip (create_pairs, match_pairs).  payne_tmatch_create leaves max_poly = 0 and max_primaries = 0 and
// both workspaces null: such a handle refuses payne_tmatch_match_poly and payne_tmatch_match_pairs.
#pragma once

struct payne_tmatch {
  int device = 0, max_stars = 0, max_templates = 0;
  double* part_c = nullptr;   // [chunks][N][topk]
  int* part_i = nullptr;
  int max_poly = 0;           // payne_tmatch_create_poly's; its workspace, per chunk of payne_tmatch_poly_chunk() templates:
  double* poly_c = nullptr;   // [chunks][N][topk]
  int* poly_i = nullptr;
  double* poly_coef = nullptr;   // [chunks][N][topk][P]
  int max_primaries = 0;      // payne_tmatch_create_pairs'; its workspace:
  double* pair_mom = nullptr;    // B [max_stars][max_templates], then S: a call indexes each as [N][M]
  double* pair_c0 = nullptr;     // [max_stars]
  double* pair_c = nullptr;      // per chunk of payne_tmatch_pair_chunk() templates [chunks][N kA][topk]
  int* pair_i = nullptr;
  double* pair_amp = nullptr;    // [chunks][N kA][topk][2]
};
