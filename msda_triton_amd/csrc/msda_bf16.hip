// msda_bf16.hip — C-ABI entry points msda_fwd_bf16 / msda_bwd_bf16 (storage type __bf16).
#include "msda_launch.hpp"

MSDA_DECLARE_RUN_VALUE_FLOAT(__bf16)  // (defined in msda_f32_sbf16.hip)

MSDA_DEFINE_ENTRY_POINTS(bf16, __bf16)
