// dynplan_host.hpp -- the host side the two planners over the learned net share (dynplan.hip, dynmppi.hip): which instantiation
// a net runs on, the dispatch to it, the persistent grid and the shape checks.  Host code only; include after side_host.hpp and
// dynplan_image.hpp (through either planner's kernels).
#pragma once

namespace {

// the compiled instantiations as tile counts, in the order of kWidths: the rule by which qsd_net_pack lays the image out
struct Tiles { int t1, t2; };
constexpr Tiles kTiles[] = {{4, 4}, {8, 8}, {13, 7}};
static_assert(16 * kTiles[0].t1 == kWidths[0][0] && 16 * kTiles[0].t2 == kWidths[0][1] && 16 * kTiles[1].t1 == kWidths[1][0] &&
              16 * kTiles[1].t2 == kWidths[1][1] && 16 * kTiles[2].t1 == kWidths[2][0] && 16 * kTiles[2].t2 == kWidths[2][1],
              "the tiles are the compiled widths");

int choose_tiles(int h1, int h2, size_t lds_bytes, Tiles *out)
{
    int pair = 0;
    if (int rc = width_pair(h1, h2, &pair)) return rc;
    const Tiles t = kTiles[pair];
    const size_t bytes = (size_t)qsd::image_layout(t.t1, t.t2).floats * sizeof(float);
    if (bytes > lds_bytes) return fail(kErrUnsupported, "the image of a (%d, %d) net (%zu bytes) does not fit in LDS", h1, h2, bytes);
    *out = t;
    return kOk;
}

template <class F>
int with_tiles_kernel(Tiles t, F &&f)
{
    if (t.t1 == 4 && t.t2 == 4) return f.template operator()<4, 4>();
    if (t.t1 == 8 && t.t2 == 8) return f.template operator()<8, 8>();
    if (t.t1 == 13 && t.t2 == 7) return f.template operator()<13, 7>();
    return fail(kErrUnsupported, "no kernel for %d x %d tiles", t.t1, t.t2);
}

// persistent grid: as many workgroups as the image lets the device hold at once (at most 4 per CU), each loads the image once;
// never more than there are groups of tiles (one wave takes a tile)
template <int T1, int T2, size_t LdsBytes>
unsigned persistent_grid(int cus, int64_t tiles_total)
{
    const int64_t groups = (tiles_total + qsd::kDynBlock / 64 - 1) / (qsd::kDynBlock / 64);
    constexpr size_t lds = (size_t)qsd::image_layout(T1, T2).floats * sizeof(float);
    constexpr int per_cu = LdsBytes / lds < 4 ? (int)(LdsBytes / lds) : 4;
    static_assert(per_cu >= 1, "image does not fit in LDS");
    const int64_t resident = (int64_t)cus * per_cu;
    return (unsigned)(groups < resident ? groups : resident);
}

int check_plan_shape(int64_t n, int horizon, int max_horizon, int paths, int max_paths)
{
    if (n <= 0) return fail(kErrInvalid, "n must be >= 1, got %lld", (long long)n);
    if (horizon < 1 || horizon > max_horizon) return fail(kErrInvalid, "horizon must be in [1, %d], got %d", max_horizon, horizon);
    if (paths < 1 || paths > max_paths) return fail(kErrInvalid, "paths must be in [1, %d], got %d", max_paths, paths);
    return kOk;
}

// -> ceil(paths / 16), the 16-candidate tiles of one env; the tiles of all envs are indexed with 31 bits
int check_plan_tiles(int64_t n, int paths, int *tiles_per_env)
{
    *tiles_per_env = (paths + 15) / 16;
    if (n > (int64_t)0x7fffffff / *tiles_per_env)
        return fail(kErrInvalid, "n * ceil(paths / 16) must be below 2^31, got %lld x %d", (long long)n, *tiles_per_env);
    return kOk;
}

}  // namespace
