// post.hip - strong-posterior post-processing of the reference's evaluation loop, on the device.
//
// Reference ops (baseline/evaluation_measures.py:203-231, utils/utils.py:146-162), per clip, host-side numpy:
//   pred = ProbabilityEncoder().binarization(pred_strong, "global_threshold", threshold=0.5)   (dcase_util: p > thr)
//   pred = scipy.ndimage.filters.median_filter(pred, (median_window, 1))                        (mode "reflect")
//   for each class column: DecisionEncoder().find_contiguous_regions(column) -> [onset, offset) frame pairs
// The reference does this one clip at a time after a batch-1 forward; here one wave owns one (clip, class) column of a
// whole batch: threshold, rank filter (for 0/1 data the median is a count), run-length decode with wave ballots.
// Output is the compact event list the host turns into the reference's DataFrame / TSV.
#include "common.h"
#include "kernels.h"
#include "post.h"

__global__ __launch_bounds__(64) void k_postprocess(const float* __restrict__ strong, int T, int NC, float threshold,
                                                    int window, uint8_t* __restrict__ binary, int32_t* __restrict__ ev_count,
                                                    int32_t* __restrict__ ev_pairs, int max_ev) {
    __shared__ uint8_t raw[PP_MAXT];
    __shared__ uint8_t flt[PP_MAXT + 1];
    const int b = blockIdx.x / NC, c = blockIdx.x % NC, lane = threadIdx.x;
    int32_t* out = ev_pairs + (size_t)blockIdx.x * max_ev * 2;
    const int n_ev = pp_decode_column(strong + (size_t)b * T * NC + c, T, NC, threshold, window, raw, flt,
                                      binary ? binary + (size_t)b * T * NC + c : nullptr,
                                      [=](int k, int frame, bool is_offset) {
                                          if (k < max_ev) out[2 * k + (is_offset ? 1 : 0)] = frame;
                                      });
    if (lane == 0) ev_count[blockIdx.x] = n_ev;
}

extern "C" int sed_postprocess(const float* strong, int n_clips, int T, int nclass, float threshold, int median_window,
                               uint8_t* binary, int32_t* ev_count, int32_t* ev_pairs, int max_events, void* stream) {
    SED_CHECK_ARG(strong && ev_count && ev_pairs, "sed_postprocess: null argument");
    SED_CHECK_ARG(n_clips >= 1 && nclass >= 1 && T >= 1 && T <= PP_MAXT, "sed_postprocess: need 1 <= T <= 2048 output frames");
    SED_CHECK_ARG(median_window >= 1 && median_window <= 63, "sed_postprocess: median_window must be in [1, 63]");
    SED_CHECK_ARG(max_events >= (T + 1) / 2, "sed_postprocess: max_events must be >= ceil(T / 2)");
    k_postprocess<<<n_clips * nclass, 64, 0, (hipStream_t)stream>>>(strong, T, nclass, threshold, median_window, binary, ev_count,
                                                                      ev_pairs, max_events);
    SED_CHECK_LAUNCH();
    return SED_OK;
}
