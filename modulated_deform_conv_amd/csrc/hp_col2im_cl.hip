// hp_col2im_cl.hip -- the storing kernels of the grad_input gather with the channels-last store policy
// (MDCONV_FLAG_GRAD_INPUT_CHANNELS_LAST): GCL = true instances of hp_col2im_kernel and hp_col2im_combine_kernel in a unit
// of their own, so that hp_col2im.hip's instances stay as they are and both compile in parallel.
#define HP_GRAD_INPUT_CL_UNIT 1
#include "hp_col2im.hip"
