// susnet_capi_episodes.hip -- susnet_episode_stats: the trainer's episode bookkeeping (the kernels: susnet_episodes.h).
#include "susnet_episodes.h"
#include "susnet_host.h"

using namespace susnet;

struct EpisodePlan {
    int32_t A, B, W;
    uint64_t carry_bytes, off_t, off_position, workspace_bytes;
};

static int episode_plan(const susnet_env *env, int64_t n_ticks, EpisodePlan &pl) {
    if (!env) return fail(SUSNET_E_INVALID, "susnet_episode_stats: null env");
    pl.A = env->c.A;
    pl.B = env->c.B;
    if (pl.A < 2 || pl.A > 12) return fail(env, SUSNET_E_INVALID, "susnet_episode_stats: 2 .. 12 agents are served");
    if (n_ticks < 1) return fail(SUSNET_E_INVALID, "susnet_episode_stats: n_ticks must be positive");
    pl.W = (pl.B + 63) / 64;
    if (n_ticks * (int64_t)pl.W > 0x7fffffffll || n_ticks * (int64_t)pl.B > (1ll << 40))
        return fail(SUSNET_E_INVALID, "susnet_episode_stats: n_ticks x batch too large for one call");
    pl.off_t = 8ull * (uint64_t)pl.A * (uint64_t)pl.B;
    pl.carry_bytes = pl.off_t + 4ull * (uint64_t)pl.B;
    pl.off_position = up(4ull * (uint64_t)n_ticks * (uint64_t)pl.W, 256);
    pl.workspace_bytes = pl.off_position + 8ull * (uint64_t)n_ticks * (uint64_t)pl.W;
    return SUSNET_OK;
}

extern "C" int susnet_episode_stats_bytes(const susnet_env *env, int32_t n_ticks, uint64_t *carry_bytes_out, uint64_t *workspace_bytes_out) {
    EpisodePlan pl;
    if (int rc = episode_plan(env, n_ticks, pl)) return rc;
    if (!carry_bytes_out || !workspace_bytes_out) return fail(SUSNET_E_INVALID, "susnet_episode_stats_bytes: null output");
    *carry_bytes_out = pl.carry_bytes;
    *workspace_bytes_out = pl.workspace_bytes;
    return SUSNET_OK;
}

template <int A>
static void episode_write_launch(const EpisodeArgs &p, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL(k_episode_write<A>, dim3(grid), dim3(kEpThreads), 0, st, p);
}

extern "C" int susnet_episode_stats(susnet_env *env, const susnet_episode_io *io, void *stream) {
    if (!env || !io) return fail(SUSNET_E_INVALID, "susnet_episode_stats: null env / io");
    EpisodePlan pl;
    if (int rc = episode_plan(env, io->n_ticks, pl)) return rc;
    if (!io->rewards || !io->done || !io->truncated || !io->roles || !io->count || !io->dropped)
        return fail(SUSNET_E_INVALID, "susnet_episode_stats: null feed array / count / dropped");
    if (io->capacity < 0 || (io->capacity > 0 && !io->log)) return fail(SUSNET_E_INVALID, "susnet_episode_stats: capacity < 0, or a capacity without a log");
    if (!(io->gamma == io->gamma)) return fail(SUSNET_E_INVALID, "susnet_episode_stats: gamma is NaN");
    if (!io->carry || io->carry_bytes < pl.carry_bytes || (reinterpret_cast<uintptr_t>(io->carry) & 7u))
        return fail(SUSNET_E_INVALID, "susnet_episode_stats: carry missing, smaller than susnet_episode_stats_bytes or not 8-byte aligned");
    if (!io->workspace || io->workspace_bytes < pl.workspace_bytes || (reinterpret_cast<uintptr_t>(io->workspace) & 7u))
        return fail(SUSNET_E_INVALID, "susnet_episode_stats: workspace missing, smaller than susnet_episode_stats_bytes or not 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(io->log) & 7u) || (reinterpret_cast<uintptr_t>(io->count) & 7u) || (reinterpret_cast<uintptr_t>(io->dropped) & 7u))
        return fail(SUSNET_E_INVALID, "susnet_episode_stats: log / count / dropped must be 8-byte aligned");
    if ((io->info == nullptr) != (io->info_log == nullptr)) return fail(SUSNET_E_INVALID, "susnet_episode_stats: info and info_log go together (both or neither)");
    if ((reinterpret_cast<uintptr_t>(io->info) & 15u) || (reinterpret_cast<uintptr_t>(io->info_log) & 15u))
        return fail(SUSNET_E_INVALID, "susnet_episode_stats: info / info_log must be 16-byte aligned");
    EpisodeArgs p;
    p.info = io->info; p.info_log = io->info_log;
    p.rewards = io->rewards; p.done = io->done; p.truncated = io->truncated; p.roles = io->roles;
    p.G = static_cast<double *>(io->carry);
    p.t_episode = reinterpret_cast<int32_t *>(static_cast<char *>(io->carry) + pl.off_t);
    p.log = io->log; p.capacity = io->capacity; p.count = io->count; p.dropped = io->dropped;
    p.counts = static_cast<int32_t *>(io->workspace);
    p.position = reinterpret_cast<int64_t *>(static_cast<char *>(io->workspace) + pl.off_position);
    p.gamma = io->gamma; p.tick_base = io->tick_base;
    p.T = io->n_ticks; p.B = pl.B; p.W = pl.W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)((pl.B + kEpThreads - 1) / kEpThreads);
    hipLaunchKernelGGL(k_episode_count, dim3(grid), dim3(kEpThreads), 0, st, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_episode_scan, dim3(1), dim3(kEpScanThreads), (kEpScanThreads / 64) * sizeof(long long), st, p);
    HIP_TRY(hipGetLastError());
    switch (pl.A) {
    case 2: episode_write_launch<2>(p, grid, st); break;
    case 3: episode_write_launch<3>(p, grid, st); break;
    case 4: episode_write_launch<4>(p, grid, st); break;
    case 5: episode_write_launch<5>(p, grid, st); break;
    case 6: episode_write_launch<6>(p, grid, st); break;
    case 7: episode_write_launch<7>(p, grid, st); break;
    case 8: episode_write_launch<8>(p, grid, st); break;
    case 9: episode_write_launch<9>(p, grid, st); break;
    case 10: episode_write_launch<10>(p, grid, st); break;
    case 11: episode_write_launch<11>(p, grid, st); break;
    default: episode_write_launch<12>(p, grid, st); break;
    }
    HIP_TRY(hipGetLastError());
    return SUSNET_OK;
}
