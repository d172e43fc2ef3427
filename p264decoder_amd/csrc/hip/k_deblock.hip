// k_deblock.hip - the loop filter's sample kernel (kernel_deblock.h: K4b) as a translation unit of its own, so that it can be
// compiled with the scheduling strategy that suits it (build.py: -mllvm -amdgpu-sched-strategy=max-ilp; see kernel_deblock.h).
// p264hip.hip declares the kernel and launches it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "p264hip.h"
#include "device_common.h"
#include "kernel_deblock.h"
