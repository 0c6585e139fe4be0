// hp_bwd2_s32.hip -- the hp_bwd2 kernels for fp32 offsets and masks (MDCONV_SAMPLING_F32): S = float instances
// in a unit of their own, so that they compile in parallel with the 16-bit ones (hp_bwd2.hip).
#define HP_SAMPLING_F32_UNIT 1
#include "hp_bwd2.hip"
