// mlp_rows_role.h — how the row kernels' launchers are cut into objects: one object per hidden
// width (NT = hidden_pad / 32, 1..8) and role. The plain kernels' objects hold exactly the
// instantiations the bench runs; the population forms of the tick and the test rollout, the
// population learner's row kernels, the BC forms of actor_rows, the population's BC form, the
// weighted form of critic_rows (prioritised replay) and the Q-filtered BC form of actor_rows live
// in objects of their own:
// compiled beside them, the plain tick kernel came out with a few scalar loads scheduled elsewhere,
// and the bench's kernels are to stay exactly as the compiler made them (tools/isa_diff.py).
// The Makefile builds mlp_rows_nt.hip once per (NAV_MLP_ROLE, NAV_MLP_PART); mlp_abi.hip calls
// the object that rows_role() names. Both sides need the launch contract (rows_args.h) and no
// device text: the launchers include that themselves (mlp_rows.h).
#pragma once
#include "rows_args.h"

// Makefile: ROLES (object name : role)
enum {
    ROLE_PLAIN = 0, ROLE_POP = 1, ROLE_LPOP = 2, ROLE_BC = 3, ROLE_BCPOP = 4, ROLE_PER = 5,
    ROLE_BCQ = 6, ROLE_COUNT = 7
};

// the role whose objects serve family `fam` (of a forward launch: with output mode `out_mode`)
constexpr int rows_role(int fam, int out_mode) {
    return fam == FAM_ACTOR_BCQ                                                   ? ROLE_BCQ
           : fam == FAM_CRITIC_W                                                  ? ROLE_PER
           : fam == FAM_ACTOR_BC_POP                                              ? ROLE_BCPOP
           : fam == FAM_ACTOR_BC                                                  ? ROLE_BC
           : fam == FAM_CRITIC_POP || fam == FAM_ACTOR_POP                       ? ROLE_LPOP
           : fam == FAM_TEST_POP || (fam == FAM_FWD && out_mode == OUT_TICK_POP) ? ROLE_POP
                                                                                 : ROLE_PLAIN;
}

// an object's dispatcher: nav_mlp_rows_<role>_<NT>(fam, rt, in_mode, out_mode, args, n_nets, st)
using rows_fn = int(int fam, int rt, int in_mode, int out_mode, const void* args, int n_nets,
                    hipStream_t st);
#define NAV_ROWS_FN2(role, nt) nav_mlp_rows_##role##_##nt
#define NAV_ROWS_FN(role, nt) NAV_ROWS_FN2(role, nt)
// X(role, nt) over one role's objects, and R(role) over the roles
#define NAV_ROWS_NTS(X, role) \
    X(role, 1) X(role, 2) X(role, 3) X(role, 4) X(role, 5) X(role, 6) X(role, 7) X(role, 8)
#define NAV_ROWS_ROLES(R) R(0) R(1) R(2) R(3) R(4) R(5) R(6)
