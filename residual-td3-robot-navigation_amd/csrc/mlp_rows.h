// mlp_rows.h — the device code of the row kernels, for the launcher objects (mlp_rows_nt.hip):
// rows_gemm.h (the hidden x hidden products), rows_layers.h (a network's forward and row backward
// over a block of rows), rows_kernels.h (k_mlp_fwd, k_test_rollout, k_mlp_bwd) and td3_rows.h
// (the fused TD3 row programs), each including what it needs, on top of the launch contract
// rows_args.h. The C ABI's object (mlp_abi.hip) includes the contract alone.
#pragma once
#include "rows_kernels.h"
#include "td3_rows.h"
