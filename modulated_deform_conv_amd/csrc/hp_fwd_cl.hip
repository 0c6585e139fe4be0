// hp_fwd_cl.hip -- the hp_fwd kernels with the channels-last store policy (MDCONV_FLAG_OUTPUT_CHANNELS_LAST): OCL = true
// instances in a unit of their own, so that hp_fwd.hip's instances stay as they are and both compile in parallel.
#define HP_OUTPUT_CL_UNIT 1
#include "hp_fwd.hip"
