// Per-element maths of the temporal terms on posed vertices of a scan sequence (include/smalfit.h, "scan sequences", the vertex
// terms): the velocity and acceleration stencils, their gradients, the element's total, the losses.  One definition each, shared by
// fit3d_sequence_vertex_kernel / fit3d_sequence_vertex_finish_kernel (kernels_mesh3d.inc) and by the test-only host shim
// (tests/host_sequence_vertex_shim.cpp).  SMALFIT_HD as in smalfit_math.h.  Every multiply-add is an explicit fmaf and no other
// expression here holds a product next to a sum, so the host (built without contraction) and the device give the same bits.
//
// THIS PROJECT'S definitions; the loss and gradient forms are those of fit3d_sequence_math.h (temporal_loss, temporal_grad).
#pragma once
#include <math.h>
#include <stddef.h>

#include "fit3d_sequence_math.h"

namespace smalfit {

// where mesh n stands in its clip [start, start + len): which of its four neighbours exist and which of the three stencil
// positions n - 1, n, n + 1 are the centre of an acceleration triple (strictly inside the clip)
struct SeqVertexPlace {
  bool has_m2, has_m1, has_p1, has_p2;      // meshes n - 2, n - 1, n + 1, n + 2 are in the clip
  bool centre_m1, centre_0, centre_p1;      // n - 1, n, n + 1 have both neighbours in the clip
};
SMALFIT_HD SeqVertexPlace sequence_vertex_place(int n, int start, int len) {
  const int end = start + len;
  SeqVertexPlace p;
  p.has_m2 = n - 2 >= start;
  p.has_m1 = n - 1 >= start;
  p.has_p1 = n + 1 < end;
  p.has_p2 = n + 2 < end;
  p.centre_m1 = p.has_m2 && p.has_m1;       // (n itself is n - 1's right neighbour)
  p.centre_0 = p.has_m1 && p.has_p1;
  p.centre_p1 = p.has_p1 && p.has_p2;
  return p;
}

// L of both terms: the elements of one mesh
SMALFIT_HD int sequence_vertex_len(int num_verts) { return 3 * num_verts; }

// the acceleration of a centre: (x[n-1] - x[n]) + (x[n+1] - x[n])
SMALFIT_HD float vertex_accel(float prev, float x, float next) { return (prev - x) + (next - x); }

// D of the velocity gradient, temporal_grad's operand order: (x - prev) + (x - next), the one-neighbour forms at the ends of a clip
SMALFIT_HD float vertex_vel_stencil(float x, float prev, float next, bool has_prev, bool has_next) {
  if (has_prev && has_next) return (x - prev) + (x - next);
  if (has_prev) return x - prev;
  if (has_next) return x - next;
  return 0.f;
}

// A of the acceleration gradient: (a[n-1] - a[n]) + (a[n+1] - a[n]), a = 0 where the mesh is no centre
SMALFIT_HD float vertex_acc_stencil(float a_prev, float a, float a_next) { return (a_prev - a) + (a_next - a); }

// one coordinate's A from the five frames x[n-2] .. x[n+2] (a frame outside the clip is never read by its flag's form)
SMALFIT_HD float vertex_acc_stencil5(const SeqVertexPlace& p, float xm2, float xm1, float x, float xp1, float xp2) {
  const float am = p.centre_m1 ? vertex_accel(xm2, xm1, x) : 0.f;
  const float a0 = p.centre_0 ? vertex_accel(xm1, x, xp1) : 0.f;
  const float ap = p.centre_p1 ? vertex_accel(x, xp1, xp2) : 0.f;
  return vertex_acc_stencil(am, a0, ap);
}

// the element's total t: fma(c_acc, A, c_vel D); an absent part is passed as c = 0 with its stencil 0
SMALFIT_HD float vertex_term_grad(float c_acc, float A, float c_vel, float D) {
  const float vel = c_vel * D;
  return fmaf(c_acc, A, vel);
}

// one element of an acceleration triple added to a running sum of squares (the velocity pair's is temporal_pair_sq)
SMALFIT_HD float vertex_accel_sq(float acc, float a) { return fmaf(a, a, acc); }

// the third entry of `losses`
SMALFIT_HD float vertex_term_total(float vel, float acc) { return vel + acc; }

// step_total of the vertex block: ((the step's total + the surface term's) + the parameter terms' sum) + the vertex terms' sum;
// `base` arrives as the first bracket
SMALFIT_HD float vertex_step_total(float base, float parameter_terms, float vertex_terms) { return (base + parameter_terms) + vertex_terms; }

}  // namespace smalfit
