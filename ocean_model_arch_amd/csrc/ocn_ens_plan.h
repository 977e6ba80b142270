// ocn_ens_plan.h -- the ensemble launch planner (ocn_sw.h ocn_ens_plan): pure host code, no HIP, so
// that it also builds into a stand-alone program (a sanitizer run of its input grid).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/ocn_sw.h"

namespace ocn {

// tiles of one member at `rows` rows per wave tile: workgroups of 4 vertically stacked waves, 60
// output columns each (sw_kernels.hip multi_tiles)
inline long ens_tiles(const ocn_block *g, int rows)
{
    const long w = (long)g->nx_end - g->nx_start + 1, h = (long)g->ny_end - g->ny_start + 1;
    return ((w + 59) / 60) * ((h + 4L * rows - 1) / (4L * rows));
}

// The policy (ocn_sw.h).  Per variant: one launch of all its members at the shortest tiles that keep
// them resident together; where even 16 rows do not, launches of capacity / tiles members at 16 rows.
// Measured on the Black Sea: one launch of taller tiles beats two or four of
// shorter ones at every member count tried, because each launch pays a barrier per step.
// Returns OCN_OK, or OCN_ERR_ARG with *err set.
inline int ens_plan_groups(const ocn_block *g, const int32_t *variant, int members, int64_t capacity,
                           std::vector<ocn_ens_group> &out, const char **err)
{
    out.clear();
    if (!g || !variant || members < 1 || members > OCN_ENS_MAX_MEMBERS || capacity < 1) {
        *err = "geometry, 1..OCN_ENS_MAX_MEMBERS members with their variants, capacity >= 1";
        return OCN_ERR_ARG;
    }
    if (g->nx_end < g->nx_start || g->ny_end < g->ny_start) {
        *err = "empty block";
        return OCN_ERR_ARG;
    }
    if (ens_tiles(g, 16) > capacity) return OCN_OK;   // (no member fits alone: none is eligible)
    std::map<int32_t, std::vector<int32_t>> by;
    for (int i = 0; i < members; ++i)
        if (variant[i] >= 0) by[variant[i]].push_back(i);
    for (const auto &kv : by) {
        const std::vector<int32_t> &ms = kv.second;
        int rows = 16;
        for (int r = 1; r <= 16; ++r)
            if ((int64_t)ms.size() * ens_tiles(g, r) <= capacity) { rows = r; break; }
        const long tiles = ens_tiles(g, rows);
        const size_t per = (size_t)std::min<int64_t>(capacity / tiles, (int64_t)ms.size());
        for (size_t i = 0; i < ms.size(); i += per) {
            ocn_ens_group q{};
            q.variant = kv.first; q.rows = rows; q.tiles = (int32_t)tiles;
            q.members = (int32_t)std::min(per, ms.size() - i);
            for (int j = 0; j < q.members; ++j) { q.member[j] = ms[i + j]; q.first_tile[j] = (int32_t)(j * tiles); }
            out.push_back(q);
        }
    }
    return OCN_OK;
}

// The recorder's schedule (ocn_sw.h ocn_ens_record_due): the 1-based steps s of a call of nsteps steps, made
// after `counted` counted steps, with (counted + s) % every == 0, in rising order
inline void ens_record_due(int64_t counted, int32_t nsteps, int32_t every, std::vector<int32_t> &out)
{
    out.clear();
    for (int64_t s = (int64_t)every - counted % every; s <= nsteps; s += every) out.push_back((int32_t)s);
}

}  // namespace ocn
