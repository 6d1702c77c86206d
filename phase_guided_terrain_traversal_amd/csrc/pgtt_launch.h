// pgtt_launch.h — what the host code (pgtt_api.hip) sees of the kernels: the argument block KArgs and the MODE_* / OBS_* enums
// (pgtt_common.hip.h), and one plain host launcher per kernel.  The kernels themselves live in pgtt_task.hip, pgtt_curriculum.hip and
// pgtt_physics_inst.hip (one translation unit per physics_kernel variant; their launchers are declared from the generated variant list).
#pragma once
#include "pgtt_common.hip.h"

// pgtt_task.hip.  observe_kernel<omode (OBS_*), a.T > 0>: one wave per env of a.N; the others one thread per env
void pgtt_launch_observe(int omode, hipStream_t st, const pgtt::KArgs& a, const float* action);
void pgtt_launch_task(hipStream_t st, const pgtt::KArgs& a, const float* action);
void pgtt_launch_reset_pose(hipStream_t st, const pgtt::KArgs& a);
void pgtt_launch_push(hipStream_t st, const pgtt::KArgs& a);
void pgtt_launch_interval_reduce(hipStream_t st, float* sums, int N, int rows, float* acc, float env_steps, int accumulate);
void pgtt_launch_variant_range(hipStream_t st, const int32_t* variant, int N, int T, int* bad);
// pgtt_curriculum.hip
int pgtt_curriculum_save_rows();
void pgtt_launch_curriculum(hipStream_t st, const pgtt::KArgs& a, const PgttCurriculum& c, unsigned char* mask, float* save);
void pgtt_launch_curriculum_restore(hipStream_t st, const pgtt::KArgs& a, const unsigned char* mask, const float* save);
void pgtt_launch_curriculum_check(hipStream_t st, const pgtt::KArgs& a, const PgttCurriculum& c, int* bad);
