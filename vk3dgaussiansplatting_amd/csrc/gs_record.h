// gs_record.h -- the layout of the 336-byte GaussianData record (Engine/Graphics/ShaderStructs.h:59-70), the unit of
// gs_upload_gaussians, of the gradients of gs_backward* and of the records, m and v of gs_adam_rows_device and
// gs_densify_device.  Host and device.  A record is 21 quads (groups of four floats):
//   quad 0      position xyz, w unused          quads 3..18  shCoeffs[k] = (r, g, b of coefficient k, w unused), except that
//   quad 1      scale xyz, w unused                          shCoeffs[0].w is the opacity
//   quad 2      rotation r, x, y, z             quads 19, 20 color, covariance: the reference's per-frame scratch, never read
// 59 of the 84 floats are fields; they all lie in the first kRecFieldQuads quads.
#pragma once

#include <stdint.h>
#include "../../include/gsplat.h"

namespace gs {

constexpr uint32_t kRecordFloats = 84, kRecordQuads = kRecordFloats / 4;
static_assert(kRecordFloats * sizeof(float) == GS_GAUSSIAN_RECORD_BYTES && kRecordQuads * 4 == kRecordFloats,
              "the record of gs_upload_gaussians is 21 quads");
constexpr uint32_t kRecPos = 0, kRecScale = 4, kRecRot = 8, kRecSh = 12, kRecOpacity = kRecSh + 3;   // float offsets
constexpr uint32_t kRecColor = 76, kRecCov = 80;
constexpr uint32_t kRecFields = 59;
constexpr uint32_t kRecFieldQuads = kRecColor / 4;          // the leading quads that hold fields
constexpr uint32_t rec_sh(uint32_t k, uint32_t c) { return kRecSh + 4u * k + c; }   // channel c of SH coefficient k
// float `col` of a record is one of the 59 fields: x, y, z of every leading quad, w of the rotation and the opacity
constexpr bool rec_is_field(uint32_t col) {
    return col < 4u * kRecFieldQuads && ((col & 3u) != 3u || col == kRecRot + 3u || col == kRecOpacity);
}

} // namespace gs
