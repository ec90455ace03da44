// The register programs of the PLONK descriptor (include/gl355.h, stark-verifier_amd/halo2.py ProgramBuilder): what the device evaluator
// (plonk_kernels.cuh) and the host interpreter (plonk_desc.h, beside the check that licenses both) read.
#pragma once
#include <stdint.h>

namespace gl355 {

constexpr uint32_t PLK_MAX_REGS = 12;        // halo2.py MAX_REGS
enum { PLK_OP_ADD = 0, PLK_OP_SUB = 1, PLK_OP_MUL = 2, PLK_OP_EMIT = 3, PLK_OP_NEG = 4, PLK_OP_MOV = 5 };
enum { PLK_K_REG = 0, PLK_K_CONST = 1, PLK_K_ADVICE = 2, PLK_K_FIXED = 3, PLK_K_INSTANCE = 4 };

}  // namespace gl355
