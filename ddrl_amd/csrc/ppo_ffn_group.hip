// The fused fcnet update of a group of contexts, as launch_update_ffn_group (ppo_ffn_impl.h built
// with DDRL_FFN_GROUP = 1): ppo_ffn.hip's row-split kernel -- the same step loop, LDS, registers and
// in-XCD exchange per chain -- with a chain axis in the grid.  One chain is one policy of one member
// context; chain c runs on blocks 32 (c >> 3) + 8 j + (c & 7), j = 0 .. 3, so up to 8 chains share
// a group row of 32 blocks and every chain's four workgroups sit on one XCD.  The chains of several
// training runs are independent, so a launch fills the CUs one run's four chains leave idle
// ("Population update").  Built with ppo_ffn.hip's flags (build.py SRC_FLAGS).
#include "kernels.h"
#if defined(DDRL_BOUNDS) || defined(DDRL_STAMPS) || defined(DDRL_XCHG_ATOMIC)
// the diagnostic libraries (bounds-checked, stamped, atomic protocol) carry no group kernel:
// ddrl_update_group_create refuses there, it never runs another kernel in its place
int update_group_grid(int n_chains) { return 32 * ((n_chains - 1) >> 3) + 24 + ((n_chains - 1) & 7) + 1; }
int launch_update_ffn_group(hipStream_t, const UpdateArgs*, int, const UpdateHyper&, int, int, int, int,
                            unsigned long long*, unsigned long long*, int*, unsigned*, int*) {
  return -1;
}
#else
#define DDRL_FFN_KSP 2
#define DDRL_FFN_GROUP 1
#include "ppo_ffn_impl.h"
#endif
