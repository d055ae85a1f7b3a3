// smalify_amd/csrc/smalfit_plan.h as C functions for tests/test_metrics_cpu.py: the rules and grids of smalfit_fit_metrics.  Built
// by g++ (tests/host_metrics.py), no HIP: the library (smalfit_launch.inc) and this shim call the same code.
#include <cstddef>

#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {
// the block is laid out by the caller (ctypes mirror of smalify_amd/_lib.py); nullptr = accepted
const char* hm_metrics_args_refusal(const smalfit_metrics_args* a, int max_frames) { return metrics_args_refusal(a, max_frames); }
int hm_sizeof_metrics_args() { return (int)sizeof(smalfit_metrics_args); }
int hm_offsetof_thresholds() { return (int)offsetof(smalfit_metrics_args, thresholds); }
int hm_max_thresholds() { return SMALFIT_MAX_PCK_THRESHOLDS; }
int hm_sil_count_pixels() { return kSilCountPixels; }
void hm_cover_grid(int F, int M, int* out) { const Grid2 g = cover_grid(F, M); out[0] = g.x; out[1] = g.y; }
void hm_sil_counts_grid(int S, int M, int* out) { const Grid2 g = sil_counts_grid(S, M); out[0] = g.x; out[1] = g.y; }
int hm_pck_grid(int M) { return pck_grid(M); }
}
