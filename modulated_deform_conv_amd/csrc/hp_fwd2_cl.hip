// hp_fwd2_cl.hip -- the hp_fwd2 kernels with the channels-last store policy (MDCONV_FLAG_OUTPUT_CHANNELS_LAST): OCL = true
// instances in a unit of their own, so that hp_fwd2.hip's instances stay as they are and both compile in parallel.
#define HP_OUTPUT_CL_UNIT 1
#include "hp_fwd2.hip"
