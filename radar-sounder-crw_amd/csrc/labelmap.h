// Label maps as the evaluation kernels read them (metrics.hip: crw_confusion; confidence.hip: crw_calibration): the two label
// dtypes and their integer codes, one lane's 16-pixel chunk as 16-byte loads, and the launch geometry of a pass over a map.  Shared
// so that the two kernels' mask and validity rules are one text: their dropped[0:2] agree on the same maps by construction.
#pragma once
#include "crw_common.h"

namespace crw {
namespace labelmap {

constexpr int CONF_BLOCK = 256;                    // 4 waves
constexpr int CONF_WAVES = CONF_BLOCK / WAVE;
constexpr int CONF_MAX_BINS = 16 * 16 + 2;
constexpr int CONF_LANE_PIX = 16;                  // pixels per lane per step
constexpr unsigned CONF_GRID = 256 * 8;            // MI355X: 256 CUs x 8 resident workgroups of 256 threads
constexpr size_t CONF_MAX_WG_PIX = (size_t)1 << 31;
constexpr int CODE_INVALID = INT32_MIN;            // a label that is no integer (NaN, 2.5, 1e30): equals no ignore label, fits no bin
constexpr int IGNORE_NONE = INT32_MIN + 1;         // "-1 = none" on the device: a code no label decodes to

inline unsigned grid_for(size_t P) {
  size_t g = (P + (size_t)CONF_BLOCK * CONF_LANE_PIX - 1) / ((size_t)CONF_BLOCK * CONF_LANE_PIX);
  if (g > CONF_GRID) g = CONF_GRID;
  const size_t need = (P + CONF_MAX_WG_PIX - 1) / CONF_MAX_WG_PIX;  // <= 2^31 pixels per workgroup
  if (g < need) g = need;
  return (unsigned)(g < 1 ? 1 : g);
}

__device__ inline int code_f32(float f) {
  int i = (f >= -16777216.f && f <= 16777216.f) ? (int)f : CODE_INVALID;  // NaN fails both comparisons
  return ((float)i == f) ? i : CODE_INVALID;
}

// 16 labels of one lane chunk -> codes
template <int DT>
struct Chunk;
template <>
struct Chunk<CRW_DT_F32> {
  float4 v[4];
  __device__ inline void load(const void *base, size_t pix) {
    const float4 *q = reinterpret_cast<const float4 *>(static_cast<const float *>(base) + pix);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  }
  __device__ inline int code(int j) const {
    const float4 &w = v[j >> 2];
    const int k = j & 3;
    return code_f32(k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w);
  }
};
template <>
struct Chunk<CRW_DT_I8> {
  int4 v;
  __device__ inline void load(const void *base, size_t pix) {
    v = *reinterpret_cast<const int4 *>(static_cast<const int8_t *>(base) + pix);
  }
  __device__ inline int code(int j) const {
    const int k = j >> 2;
    const int w = k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
    return (int)(int8_t)(w >> (8 * (j & 3)));
  }
};
struct NoChunk {
  __device__ inline void load(const void *, size_t) {}
  __device__ inline int code(int) const { return CODE_INVALID; }  // never equals an ignore label
};

__device__ inline int code_at(const void *base, int dt, size_t i) {
  return dt == CRW_DT_F32 ? code_f32(static_cast<const float *>(base)[i]) : (int)static_cast<const int8_t *>(base)[i];
}

inline bool dtype_ok(int dt) { return dt == CRW_DT_F32 || dt == CRW_DT_I8; }
inline size_t elem(int dt) { return dt == CRW_DT_F32 ? 4 : 1; }

}  // namespace labelmap
}  // namespace crw
