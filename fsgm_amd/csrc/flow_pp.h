// flow_pp.h -- what the filtered-flow pipeline (capi_flow_pp.hip) borrows from the two pyramidal drivers: the cached plan of
// batch 2n of either matcher, under its device lock (pyramid_driver.h: PyramidPair, pyramid_with_pair)
#pragma once
#include "pyramid_driver.h"
#include <functional>

namespace fsgm {

using PairBody = std::function<fsgm_status(const PyramidPair&)>;
// ru: the plan with the runner-up switch on (PyramidPair::minC2 is set); lm: its level median (0, 3 or 5); each combination is a
// cached plan of its own
fsgm_status pyd_pyramid_with_pair(int n, int W, int H, int channels, const fsgm_pyramid_params* prm, int ru, int lm, const PairBody& body);   // capi_pyramid.hip
fsgm_status ng_pyramid_with_pair(int n, int W, int H, int channels, const fsgm_ng_pyramid_params* prm, int ru, int lm, const PairBody& body);  // capi_ng_pyramid.hip

}  // namespace fsgm
