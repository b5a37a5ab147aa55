// The fused fcnet update for sgd_minibatch_size = 256, as launch_update_ffn_mb256 (ppo_ffn_impl.h
// built with DDRL_MB = 256): the row split of ppo_ffn.hip with 128 rows per workgroup -- four
// waves of two 16-row tiles each, the geometry of the split-less A = 8 kernel -- so the partner
// exchange, the norm exchange, the barriers and Adam are paid once per 256 rows.  The exchange
// (two parties, LSB-tagged quads, 256 lanes) and the placement of blocks p + 8 j are those of the
// 128-row kernels.  The policy head's gradient is reduced with DPP transposes: the two
// feature-major images of ppo_ffn.hip's matrix-core form do not fit LDS at 128 rows.
// DESIGN.md section 3, "256-row minibatches", has the LDS table, the registers and the measurement.
#define DDRL_MB 256
#define DDRL_FFN_KSP 2
#include "ppo_ffn_impl.h"
