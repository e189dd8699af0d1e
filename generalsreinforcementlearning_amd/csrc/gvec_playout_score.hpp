// gvec_playout_score.hpp — the value of one playout row (PlayoutScore.__call__ of search.py, operation for operation), its
// one definition on the device: gvec_search_halve's round tail (gvec_halving.hip) and gvec_tree_backup (gvec_tree.hip) score with
// it.  The build's -ffp-contract=off keeps the products and sums apart.  W: an argument struct with win, loss, land, army.
#pragma once
#include <stdint.h>

namespace gvec {

__device__ __forceinline__ double playout_ratio(double mine, double others) {
  const double den = mine + others;
  return den != 0.0 ? mine / den : 0.5;
}
template <typename W>
__device__ __forceinline__ double playout_score(const W& P, const int32_t* __restrict__ t) {
  const double shaped = (P.land * playout_ratio((double)t[4], (double)t[6]) + P.army * playout_ratio((double)t[5], (double)t[7])) -
                        (P.land + P.army) / 2.0;
  const double lost = t[2] == 0 ? P.loss : shaped;
  return t[3] != 0 ? P.win : lost;
}

}  // namespace gvec
