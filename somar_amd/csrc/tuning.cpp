// somar_amd/csrc/tuning.cpp -- see tuning.h.  One row per switch, in the order of the table of DESIGN.md 8.9.
#include "tuning.h"

#include <cstdlib>
#include <cstring>
#include <string>

namespace somar {

namespace {
// how a variable that is SET becomes the field's value (unset: the field keeps its default)
enum Rule {
    PRESENT,   // 1, whatever the text (=0 switches it on too)
    NONZERO,   // atoi != 0
    COUNT,     // atoll
    INT,       // atoi
    ONLY,      // atoi == alt ? alt : the default
};
struct Switch { const char* name; long long Tuning::*field; Rule rule; int alt; };
const Switch SWITCHES[] = {
    {"FUSED_MIN_CELLS", &Tuning::fused_min_cells, COUNT, 0},
    {"MARCH_MIN_CELLS", &Tuning::march_min_cells, COUNT, 0},   // unset: fused_min_cells (below)
    {"FUSED_ROWS", &Tuning::fused_rows, ONLY, 8},
    {"FULL_ROWS", &Tuning::full_rows, ONLY, 6},
    {"NO_BALANCED_TILES", &Tuning::no_balanced_tiles, PRESENT, 0},
    {"NO_NARROW_TILES", &Tuning::no_narrow_tiles, PRESENT, 0},
    {"NARROW_7PT", &Tuning::narrow_7pt, NONZERO, 0},           // tri-state: unset stays -1
    {"NO_LEAN_TILES", &Tuning::no_lean_tiles, PRESENT, 0},
    {"NO_UNIFORM", &Tuning::no_uniform, NONZERO, 0},
    {"NO_ZERO_PLANES", &Tuning::no_zero_planes, NONZERO, 0},
    {"NO_ZERO_START", &Tuning::no_zero_start, PRESENT, 0},
    {"NO_FOLD_PROLONG", &Tuning::no_fold_prolong, PRESENT, 0},
    {"NO_CF_FUSED", &Tuning::no_cf_fused, PRESENT, 0},
    {"AMR_PLAIN", &Tuning::amr_plain, NONZERO, 0},
    {"FUSED_BOTTOM_MAX_CELLS", &Tuning::fused_bottom_max_cells, COUNT, 0},
    {"BOX_BOTTOM", &Tuning::box_bottom, NONZERO, 0},
    {"BOX_BOTTOM_MIN_CELLS", &Tuning::box_bottom_min_cells, COUNT, 0},
    {"BOX_TIMING", &Tuning::box_timing, PRESENT, 0},
    {"BOTTOM_ASYNC", &Tuning::bottom_async, NONZERO, 0},
    {"ORDERED_REDUCE_MAX", &Tuning::ordered_reduce_max, COUNT, 0},
    {"ORDERED_SERIAL", &Tuning::ordered_serial, PRESENT, 0},
    {"NO_FUSED_PUBLISH", &Tuning::no_fused_publish, PRESENT, 0},
    {"POLL_FETCH", &Tuning::poll_fetch, NONZERO, 0},           // on unless set to 0
    {"GHOST_STAGED", &Tuning::ghost_staged, NONZERO, 0},
    {"NO_GHOST_DCE", &Tuning::no_ghost_dce, PRESENT, 0},
    {"FLUX_FIELDS", &Tuning::flux_fields, PRESENT, 0},
    {"FUSED19_MIN_BOX", &Tuning::fused19_min_box, INT, 0},
    {"CF_FULL_GATHER", &Tuning::cf_full_gather, PRESENT, 0},
    {"PULL_MAX_CELLS", &Tuning::pull_max_cells, COUNT, 0},
    {"GRAPH_CELLS", &Tuning::graph_cells, COUNT, 0},
    {"AGGLOM_CELLS", &Tuning::agglom_cells, COUNT, 0},
    {"NO_OVERLAP", &Tuning::no_overlap, NONZERO, 0},
    {"TIMING", &Tuning::timing, INT, 0},
};
}  // namespace

Tuning Tuning::from_env()
{
    Tuning t;
    bool march_set = false;
    for (const Switch& s : SWITCHES) {
        const char* e = getenv((std::string("SOMAR_") + s.name).c_str());
        if (!e) continue;
        long long& v = t.*s.field;
        switch (s.rule) {
            case PRESENT: v = 1; break;
            case NONZERO: v = atoi(e) != 0; break;
            case COUNT: v = atoll(e); break;
            case INT: v = atoi(e); break;
            case ONLY: if (atoi(e) == s.alt) v = s.alt; break;
        }
        if (s.field == &Tuning::march_min_cells) march_set = true;
    }
    if (!march_set) t.march_min_cells = t.fused_min_cells;
    // the staged-coefficient sweep's two switches are read here, not from the table: the table is the list that
    // DESIGN.md 8.9 and tests/test_gpu_tuning.py pin row for row
    if (const char* e = getenv("SOMAR_NO_STAGED_COEF")) t.no_staged_coef = atoi(e) != 0;
    if (const char* e = getenv("SOMAR_STAGED_MIN_CELLS")) t.staged_min_cells = atoll(e);
    return t;
}

bool Tuning::get(const char* name, long long* value) const
{
    for (const Switch& s : SWITCHES)
        if (!strcmp(name, s.name)) { *value = this->*s.field; return true; }
    if (!strcmp(name, "NO_STAGED_COEF")) { *value = no_staged_coef; return true; }
    if (!strcmp(name, "STAGED_MIN_CELLS")) { *value = staged_min_cells; return true; }
    return false;
}

}  // namespace somar
