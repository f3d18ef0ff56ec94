// row_parts.h -- the rows of a bank or a panel cut into parts, one workgroup (per query or problem tile) each: the host plan that the
// planners of knn.hip, agg.hip and probe.hip share, and the range a kernel takes from it.  Internal: not part of the C ABI.
#pragma once
#include <algorithm>

namespace avae {

struct RowParts { int parts, chunk; };

// N >= 1 rows cut into `parts` runs of `chunk` rows.  chunk is a multiple of `tile` -- enough tiles per part for `want` parts -- unless
// chunk_opt > 0 gives it (a test aid: parts that are no tile multiple).  Either is raised to the next tile multiple that keeps the
// part count within max_parts, and is at most 0x7fffff80 (an int, and a multiple of every tile here).
inline RowParts row_parts(long long N, int tile, int want, int max_parts, int chunk_opt)
{
    if (N < 1) return RowParts{0, 0};
    long long chunk;
    if (chunk_opt > 0) chunk = chunk_opt;
    else {
        const long long tiles = (N + tile - 1) / tile, w = std::max(want, 1);
        chunk = ((tiles + w - 1) / w) * tile;
    }
    if ((N + chunk - 1) / chunk > max_parts) chunk = (((N + max_parts - 1) / max_parts + tile - 1) / tile) * tile;
    RowParts r;
    r.chunk = (int)std::min<long long>(chunk, 0x7fffff80);
    r.parts = (int)((N + r.chunk - 1) / r.chunk);
    return r;
}

#if defined(__HIPCC__)
// rows [begin, end) of part `part`: begin is 64-bit (part * chunk may pass 2^31 in the last, clamped part of a 2^31 - 256 row call),
// end <= N is not
__device__ __forceinline__ void part_range(int part, int chunk, int N, long long& begin, int& end)
{
    begin = (long long)part * chunk;
    end = begin + chunk < (long long)N ? (int)(begin + chunk) : N;
}
#endif

}  // namespace avae
