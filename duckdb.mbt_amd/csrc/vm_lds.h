// vm_lds.h — the tile interpreter's register file and loop, shared by the
// units whose kernels interpret a VM program (kernels.hip: the filter /
// project passes; join_kernels.hip: the fused probe-and-aggregate).
//
// VM register planes [reg][row] in dynamic LDS sized to the program's
// register count (P.n_regs), not VM_MAX_REGS: short programs leave room for
// more resident workgroups, i.e. more row loads in flight per CU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vm.h"
#include "vm_device.h"

namespace mbx {
namespace dev {

struct VmLds {
  int64_t *lo;
  int64_t *hi;
  uint8_t *nl;
};
__device__ __forceinline__ VmLds vm_regs(unsigned char *base, int n_regs) {
  VmLds R;
  R.lo = (int64_t *)base;
  R.hi = R.lo + (size_t)n_regs * VM_TILE;
  R.nl = (uint8_t *)(R.hi + (size_t)n_regs * VM_TILE);
  return R;
}
static inline size_t VmLdsBytes(int n_regs) { return (size_t)(n_regs < 1 ? 1 : n_regs) * VM_TILE * 17; }

// LDS-plane register file of the tile interpreter
struct LdsRF {
  const VmLds &R;
  int t;
  __device__ __forceinline__ int64_t &lo(int i) { return R.lo[i * VM_TILE + t]; }
  __device__ __forceinline__ int64_t &hi(int i) { return R.hi[i * VM_TILE + t]; }
  __device__ __forceinline__ uint8_t &nl(int i) { return R.nl[i * VM_TILE + t]; }
};

// the whole program for the calling thread's row
__device__ inline void vm_exec(const VmProgram &P, const VmCols &C, int64_t row, bool active, int64_t rs,
                               int64_t rstep, const VmLds &R, int t, int32_t *err) {
  LdsRF rf{R, t};
  for (int k = 0; k < P.n_ins; k++) {
    const VmIns I = P.ins[k];
    vm_step(P, C, I.op, I.dst, I.a, I.b, I.c, I.aux, row, active, rs, rstep, rf, err);
  }
}

}  // namespace dev
}  // namespace mbx
