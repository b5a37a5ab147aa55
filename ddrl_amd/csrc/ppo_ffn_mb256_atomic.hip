// ppo_ffn_mb256.hip with the atomic exchange protocol of ppo_ffn_atomic.hip, as
// launch_update_ffn_mb256_atomic: what a sgd_minibatch_size = 256 context switches to when the
// placement check fails or DDRL_XCHG=atomic is set.
#define DDRL_MB 256
#define DDRL_FFN_KSP 2
#define DDRL_FFN_AT 1
#include "ppo_ffn_impl.h"
