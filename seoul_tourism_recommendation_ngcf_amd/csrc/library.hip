// library.hip - what belongs to the library as a whole: its identity, the option table, the launch timing of the SpMM.
#include "common.h"

extern "C" const char *ngcf_last_error(void) { return g_err; }
extern "C" const char *ngcf_target_arch(void) { return "gfx950"; }
extern "C" int ngcf_version(void) { return NGCF_ABI_VERSION; }   // the mirror refuses a library built from another header

// ---------------------------------------------------------------------------------------------
// options (common.h, NgcfOptions): the ONLY place of the library that reads the environment
// ---------------------------------------------------------------------------------------------
NgcfOptions g_opts;

namespace {
struct OptField {
    const char *name;       // option name = environment variable without the NGCF_ prefix, lower case
    int NgcfOptions::*i;
    int64_t NgcfOptions::*l;
};
const OptField kOptFields[] = {
    {"no_fork", &NgcfOptions::no_fork, nullptr},
    {"no_slicing", &NgcfOptions::no_slicing, nullptr},
    {"no_ldstab", &NgcfOptions::no_ldstab, nullptr},
    {"no_panel_split", &NgcfOptions::no_panel_split, nullptr},
    {"no_tail_table", &NgcfOptions::no_tail_table, nullptr},
    {"no_pad_product", &NgcfOptions::no_pad_product, nullptr},
    {"fork_min", nullptr, &NgcfOptions::fork_min},
    {"dense_direct", &NgcfOptions::dense_direct, nullptr},
    {"dense_resident", &NgcfOptions::dense_resident, nullptr},
    {"dense_resident_min_rows", &NgcfOptions::dense_resident_min_rows, nullptr},
    {"dense_small_tiles", &NgcfOptions::dense_small_tiles, nullptr},
    {"dense_tall", &NgcfOptions::dense_tall, nullptr},
    {"bwd_input_resident", &NgcfOptions::bwd_input_resident, nullptr},
    {"t_rows_bitmap", &NgcfOptions::t_rows_bitmap, nullptr},
    {"select_no_lds", &NgcfOptions::select_no_lds, nullptr},
    {"slice_max_mb", &NgcfOptions::slice_max_mb, nullptr},
    {"swept_lpe", &NgcfOptions::swept_lpe, nullptr},
    {"swept_cut", &NgcfOptions::swept_cut, nullptr},
    {"swept_no_moments", &NgcfOptions::swept_no_moments, nullptr},
    {"swept_order_rows", &NgcfOptions::swept_order_rows, nullptr},
    {"swept_debug", &NgcfOptions::swept_debug, nullptr},
    {"swept_window_kb", &NgcfOptions::swept_window_kb, nullptr},
    {"swept_spin", &NgcfOptions::swept_spin, nullptr},
    {"swept_lead", &NgcfOptions::swept_lead, nullptr},
    {"swept_sync_every", &NgcfOptions::swept_sync_every, nullptr},
    {"swept_prio_kb", &NgcfOptions::swept_prio_kb, nullptr},
    {"swept_prio_graded", &NgcfOptions::swept_prio_graded, nullptr},
};
bool g_opts_read = false;
}  // namespace

// Defaults, then every NGCF_<NAME> variable that is set (a flag variable that is set but empty counts as 1).  Called once on
// first use; tools call it again after changing os.environ.
extern "C" int ngcf_options_from_env(void)
{
    NgcfOptions o;
    for (const OptField &f : kOptFields) {
        char var[64] = "NGCF_";
        size_t n = strlen(var);
        for (const char *p = f.name; *p && n + 1 < sizeof(var); ++p) var[n++] = (char)((*p >= 'a' && *p <= 'z') ? *p - 32 : *p);
        var[n] = 0;
        const char *e = getenv(var);
        if (!e) continue;
        const long long v = *e ? atoll(e) : 1;
        if (f.i) o.*(f.i) = (int)(*e && (*e == '-' || (*e >= '0' && *e <= '9')) ? v : 1);
        else o.*(f.l) = v;
    }
    if (const char *e = getenv("NGCF_SWEPT_ORDER")) o.swept_order_rows = !strcmp(e, "rows");
    g_opts = o;
    g_opts_read = true;
    return NGCF_OK;
}

const NgcfOptions &ngcf_opts()
{
    if (!g_opts_read) ngcf_options_from_env();
    return g_opts;
}

extern "C" int ngcf_set_option(const char *name, int64_t value)
{
    if (!name) return fail(NGCF_ERR_ARG, "ngcf_set_option: null name");
    (void)ngcf_opts();
    for (const OptField &f : kOptFields)
        if (!strcmp(f.name, name)) {
            if (f.i) g_opts.*(f.i) = (int)value;
            else g_opts.*(f.l) = value;
            return NGCF_OK;
        }
    return fail(NGCF_ERR_ARG, "ngcf_set_option: unknown option '%s'", name);
}

// ---------------------------------------------------------------------------------------------
// optional in-library timing of the dominant kernel (bench.py's roofline figure): when enabled,
// a hipEvent pair is recorded on the launch stream around every spmm_kernel launch.
// ---------------------------------------------------------------------------------------------
static bool g_prof_on = false;
static std::vector<hipEvent_t> g_prof_events;   // pairs: begin, end
static size_t g_prof_used = 0;

void prof_mark(hipStream_t stream, int which)
{
    if (!g_prof_on) return;
    if (g_prof_used >= g_prof_events.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        g_prof_events.push_back(e);
    }
    (void)which;
    (void)hipEventRecord(g_prof_events[g_prof_used++], stream);
}

extern "C" int ngcf_prof_enable(int on)
{
    g_prof_on = on != 0;
    g_prof_used = 0;
    return NGCF_OK;
}

// Waits for the recorded events; returns the number of timed spmm launches and their summed duration.
extern "C" int ngcf_prof_collect(int64_t *n_launches, double *total_ms)
{
    if (!n_launches || !total_ms) return fail(NGCF_ERR_ARG, "prof_collect: null argument");
    double sum = 0.0;
    int64_t n = 0;
    for (size_t i = 0; i + 1 < g_prof_used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(g_prof_events[i + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, g_prof_events[i], g_prof_events[i + 1]));
        sum += ms;
        ++n;
    }
    *n_launches = n;
    *total_ms = sum;
    g_prof_used = 0;
    return NGCF_OK;
}
