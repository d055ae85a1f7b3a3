// TEST-ONLY host build (g++) of the window-row rules of smalify_amd/csrc/smalfit_plan.h: extern "C" wrappers over the very
// functions smalfit_fit_eval_windows calls before it launches anything.  Never part of the product.
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {

int wr_sizeof_window_rows(void) { return (int)sizeof(smalfit_window_rows); }
int wr_row_floats(int which) { return which == 0 ? kWindowRowBetas : kWindowRowScales; }
int wr_window_rows_count(int window, int frame_offset, int M) { return window_rows_count(window, frame_offset, M); }
int wr_prior_windows(int window, int frame_offset, int M) { return prior_windows(window, frame_offset, M); }
const char* wr_window_rows_size_refusal(const smalfit_window_rows* r) { return window_rows_size_refusal(r); }
// what the entry point does with the two blocks, in its order: the rows' size, the fit block, the rows
const char* wr_refusal(const smalfit_fit_args* a, const smalfit_window_rows* r, int max_frames, int has_pose_prior, int shape_dim) {
  if (const char* msg = window_rows_size_refusal(r)) return msg;
  if (const char* msg = fit_args_refusal(a, EngineFacts{max_frames, has_pose_prior != 0, shape_dim})) return msg;
  return window_rows_refusal(a, r);
}

}  // extern "C"
