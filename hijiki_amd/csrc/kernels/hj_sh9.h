// The real spherical-harmonic basis of bands 0..2 - the ONE text of it: the gather's SH reduction (api/gather_query.hip, k_gq_resolve)
// weights a sample's radiance with it, the probe look-up (kernels/hj_probes.h, k_pv_sample) evaluates a volume's coefficients with it.
// A header of its own, beside hj_num.h alone, so that neither unit's machine code depends on the other's kernels.
#pragma once
#include "hj_num.h"

#pragma clang fp contract(off)

namespace hj {

// The basis at d (not renormalised), in the order and with the constants and operation order of include/hijiki_hip.h:
// 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2
HJ_DEV void sh9_basis(v3 d, float (&Y)[9]) {
  constexpr float c0 = 0x1.20dd76p-2f, c1 = 0x1.f45438p-2f, c2 = 0x1.17b142p+0f, c3 = 0x1.42f602p-2f, c4 = 0x1.17b142p-1f;
  Y[0] = c0;
  Y[1] = c1 * d.y;
  Y[2] = c1 * d.z;
  Y[3] = c1 * d.x;
  Y[4] = c2 * (d.x * d.y);
  Y[5] = c2 * (d.y * d.z);
  Y[6] = c3 * ((3.0f * d.z) * d.z - 1.0f);
  Y[7] = c2 * (d.x * d.z);
  Y[8] = c4 * (d.x * d.x - d.y * d.y);
}

}  // namespace hj
