// The sweep launch's grid and role decode (smalify_amd/csrc/smalfit_plan.h) for tests/test_sweep_grid_cpu.py: the functions
// the host sizes the launch by and raster_sweep_kernel decodes its workgroup's role by, as C calls.
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {

// out5: frame riders | sweep blocks | joint riders | the launch's grid | sweep blocks per frame
void hs_sweep_launch_grid(int F, int M, int joints, int* out5) {
  out5[0] = box_frame_blocks(M);
  out5[1] = sweep_grid(F, M);
  out5[2] = box_joint_blocks(M, joints != 0);
  out5[3] = sweep_launch_grid(F, M, joints != 0);
  out5[4] = sweep_blocks_per_frame(F);
}

// out3: role (0 frame rider, 1 faces, 2 joint rider) | frame | block of the frame / joint
void hs_sweep_block_at(int b, int F, int M, int* out3) {
  const SweepBlock s = sweep_block_at(b, F, M);
  out3[0] = (int)s.role; out3[1] = s.n; out3[2] = s.bx;
}

// the decode of every workgroup of a launch at once: out[3 b ..]
void hs_sweep_blocks(int F, int M, int joints, int* out) {
  const int grid = sweep_launch_grid(F, M, joints != 0);
  for (int b = 0; b < grid; ++b) hs_sweep_block_at(b, F, M, out + 3 * b);
}

void hs_xcd_block_at(int b, int blocks_per_frame, int* out2) {
  const XcdBlock x = xcd_block_at(b, blocks_per_frame);
  out2[0] = x.n; out2[1] = x.bx;
}

int hs_joint_blocks() { return kJointBlocks; }

}  // extern "C"
