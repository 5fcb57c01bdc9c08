// hydrocol.hip -- C-ABI (include/hydrocol.h) and kernel launches for gfx950.
// Host side is plain C++ over the HIP runtime; nothing here falls back to the CPU.
#include "../../include/hydrocol.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hc_launch.h"

using namespace hc;

// layouts the ctypes binding (hydromodel_amd/_lib.py) mirrors; tests/test_abi.py checks the Python side
static_assert(sizeof(hc_column_params) == 8 * 4 + 15 * 8 + 2 * 4, "hc_column_params layout");
static_assert(sizeof(hc_step_args) == 8 + 8 + 4 + 4 + 5 * 8 + 8 + 8, "hc_step_args layout");
static_assert(sizeof(hc_spinup_args) == 8 + 4 + 4 + 8 + 8 + 8 + 8, "hc_spinup_args layout");

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(HC_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                \
    } while (0)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    int ensure(size_t count)
    {
        if (count <= n && p) return HC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        if (count == 0) return HC_OK;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T)));
        n = count;
        return HC_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// A table the handle accumulates over the members -- the per-row water-table moments, the profile statistics, the
// water-table and soil-moisture histograms: its device buffer and the shape key it was made for.  `ensure` re-creates it, zeroed, when the
// key changed or after `invalidate`.
template <typename T>
struct AccTable {
    const char *unit;            // what a size check counts: "words" or "entries"
    DevBuf<T> buf;
    int64_t key[3] = {-1, -1, -1};   // (key[0] = -1: no table)
    int64_t n = 0;               // entries of the current table
    int ensure(int64_t k0, int64_t k1, int64_t k2, int64_t count)
    {
        if (key[0] == k0 && key[1] == k1 && key[2] == k2) return HC_OK;
        if (buf.ensure((size_t)count)) return HC_ERR_DEVICE;
        HIP_TRY(hipMemset(buf.p, 0, (size_t)count * sizeof(T)));
        key[0] = k0, key[1] = k1, key[2] = k2;
        n = count;
        return HC_OK;
    }
    void invalidate() { key[0] = -1; }
    void release() { buf.release(), invalidate(); }
};

// A filter's soil-moisture record (hc_set_filter_soil_moisture, hc_set_enkf_soil_moisture) on the host: nodes, sigma and
// values [rows][n] (NaN = none); its diagnostics float64 [P][n_arow][n][6], keyed like the owner's table.  `width` is
// the owner's own account of its last assimilation: the particle filter's m_s (0 = it took the bin path), the EnKF's
// m' = 1 + m_s (0 = no sensor on it).
struct SmRecord {
    int n = 0;                   // 0: no record
    int64_t rows = 0;
    std::vector<int> nodes;
    std::vector<double> sigma, values;
    int width = 0;
    AccTable<double> table{"entries"};
    void clear()
    {
        n = width = 0;
        rows = 0;
        nodes.clear(); sigma.clear(); values.clear();
        table.release();
    }
};

// The well's record inside a filter's window (hc_set_filter_window, hc_set_enkf_window): the offsets, ascending; what
// the owner keeps per member of the lagged rows, `cap` [n][N] (the particle filter: water-table indices, the EnKF: y),
// and the row each slot holds (-1: none; cleared by the assimilation); diagnostics float64 [P][n_arow][n][4], keyed
// like the owner's table; the last assimilation's lagged columns (their slots, in column order)
struct WindowBase {
    int n = 0;                   // 0: no window
    std::vector<int> off;
    std::vector<int64_t> row;
    std::vector<int> last;
    AccTable<double> table{"entries"};
};
template <typename T>
struct Window : WindowBase {
    DevBuf<T> cap;
    void clear()
    {
        n = 0;
        off.clear(); row.clear(); last.clear();
        table.release();
        cap.release();
    }
};

// What the EnKF keeps, per point, of a vector x [N][D] it analyses (the state psi, the members' noise vectors z), of the
// last analysis (test hooks) and sized by the record's largest m', Wx: the raw sums of both prior passes over (x, Y),
// s1 [P][D + m'] and s2 [P][s2_cols]; the gain [P][m'][D]; for the square-root scheme the reduced gain [P][m'][D] and
// the mean's increment [P][D]; where the spread is wanted the sums of the squared anomalies before / after the update
// and of the analysed columns, [P][D] each; where x is relaxed (sigma_b, sigma_a, f, the analysis's mean) [4][P][D]
struct EnkfVec {
    DevBuf<double> s1, s2, gain, rgain, dbar, sq_b, sq_a, mean_a, relax;
    int ensure(int64_t P, int64_t D, int64_t Wx, int64_t s2_cols, bool root, bool spread, bool relaxed)
    {
        const size_t PD = (size_t)(P * D), PWD = (size_t)(P * Wx * D);
        if (s1.ensure((size_t)(P * (D + Wx))) || s2.ensure((size_t)(P * s2_cols)) || gain.ensure(PWD) ||
            (root && (rgain.ensure(PWD) || dbar.ensure(PD))) || (relaxed && relax.ensure(4 * PD)) ||
            (spread && (sq_b.ensure(PD) || sq_a.ensure(PD) || mean_a.ensure(PD))))
            return HC_ERR_DEVICE;
        return HC_OK;
    }
    void release() { for (auto *b : {&s1, &s2, &gain, &rgain, &dbar, &sq_b, &sq_a, &mean_a, &relax}) b->release(); }
};

}  // namespace

struct hc_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool have_column = false, have_forcing = false, have_noise = false;
    hc_column_params p{};        // parameter point 0; dim_d, n_groups and dz are shared by every point
    ColumnDev P{};               // point 0
    int cpl = 0, wpb = 0, slots = 0;
    bool special = false;        // every point is vrettas_fung with n = 2, m = 1/2, lambda = 1
    bool force_generic = false;  // hc_set_generic_exponents: never take the specialised cell model
    bool use_special() const { return special && !force_generic; }
    // parameter points (BASELINE config 5): host copies, uploaded by fill_args when `points_dirty`
    int n_points = 0;
    std::vector<ColumnDev> P_host;
    std::vector<double> tab_host, node_host;
    bool points_dirty = false;
    // split column (two waves per member, hc_device.h Comm<2>): columns of 513..640 nodes with one parameter point and
    // the root zone inside the upper half; its own slot layout of the tables (point 0 only)
    // HYDROCOL_SPLIT_COLUMN=0 keeps the one-wave kernels, =1 takes the split column wherever it applies (A/B, cross-checks).
    // Round 4 default: the split column from 10 cells per lane on (D = 577..640); the one-wave kernel of 9 cells per lane
    // (global region behind a buffer resource) had overtaken it at D = 513..576 (97.0 k against 95.7 k column-days/s).
    // Round 5: the split column on the TWO layout -- four pairs per CU -- runs 125 k at every depth it serves (generic
    // exponents 73 k) and is the default from 513 nodes on (use_pair below; profiles/r05_split_column_two.txt)
    bool pair_ok = false, no_split = false, force_split = false;
    std::vector<double> tab_pair_host;
    DevBuf<double> tab_pair;
    DevBuf<int> gtab_pair;
    // (round 5: the split column runs on the TWO layout, four pairs per CU -- 125 k column-days/s at D = 513 ... 640 against
    //  96 k of the one-wave kernel of 9 cells per lane at D = 541 -- so it is the default from 513 nodes on)
    bool use_pair() const { return pair_ok && !no_split && (force_split || cpl >= 9); }
    // HYDROCOL_MODEL_PACK=0: the 5-cells-per-lane step kernel never takes its packed cell model (ColumnDev::flag_pack; A/B,
    // cross-checks: the same binary, the same bits)
    bool model_pack = true;
    // HYDROCOL_JAC_LOCAL3=0: the same kernel always evaluates the host's column groups for its FD Jacobian, never the three
    // groups i % 3 on rows with a local RHS (ColumnDev::flag_jac3; A/B, cross-checks: the same binary, the same bits)
    bool jac_local3 = true;
    int chunk_members = 0;      // HYDROCOL_CHUNK_MEMBERS (0: derived from the member count)
    DevBuf<double> tab, node_tabs, precip, atm, psi, base, nscale, fresh, psi_rows, scratch_d, diag;
    DevBuf<double> wave_spill;   // per-wave vectors of deep columns that do not fit in LDS (hc_step.h WaveVecs)
    DevBuf<int> spin_iters;
    DevBuf<double> trace;        // diagnostic builds only
    int max_phase_iterations = MAX_PHASE_ITERATIONS;
    int scipy_152 = 0;           // hc_set_scipy_152
    bool strict_guard = false;   // HYDROCOL_STRICT_GUARD=1: a tripped iteration guard fails the call
    DevBuf<int> gtab, wtd_obs, draw_idx, stats, scratch_i;
    DevBuf<unsigned char> daylight, refresh;
    DevBuf<unsigned short> wtd_u16;
    AccTable<long long> moments{"words"};     // [P][3][T], keyed by the point count, reset by hc_set_forcing
    DevBuf<unsigned long long> counters;
    DevBuf<ColumnDev> Pdev;
    DevBuf<IoArgsExt> iodev;
    // several parameter points: Philox key of each point's first member, walk order of the chunk ticket, per-point cost
    DevBuf<long long> point_base;
    DevBuf<int> point_order;
    DevBuf<unsigned long long> point_cost;
    std::vector<long long> base_host;            // set by hc_set_point_member_bases (empty: member_offset + k * members_per_point)
    std::vector<int> order_host;
    bool fixed_order = false;                    // HYDROCOL_POINT_ORDER=fixed: keep the walk in point order (A/B timing)
    std::vector<unsigned long long> cost_total;  // RHS evaluations per point since the points were installed
    IoArgsExt io_host{};
    std::vector<unsigned char> h_refresh;
    int64_t n_rows = 0, n_members = 0;
    bool philox = false;
    uint64_t seed = 0;
    int64_t member_offset = 0;
    int rows_per_launch = 0;     // 0: chosen from the member count (auto_rows_per_launch)
    // ensemble profile statistics (hc_set_profile_stats): one int64 table, layout in include/hydrocol.h, keyed by
    // (points, rows, depth)
    int prof_stride = 0;         // 0: off
    AccTable<long long> prof{"words"};
    // ensemble water-table histograms (hc_set_wtd_hist): int32 [P][n_hrow][D], keyed like the profile table
    int hist_stride = 0;         // 0: off
    AccTable<int> hist{"entries"};
    // ensemble soil-moisture histograms (hc_set_theta_hist): int32 [P][n_prow][D][B] and the outside count in two more
    // entries, on the profile rows and keyed like the profile table
    int thist_bins = 0;          // 0: off
    AccTable<int> thist{"entries"};
    // ensemble soil-water storage by depth layer (hc_set_layer_storage): the int64 moments [P][n_prow][L][5], scnt, ovf and,
    // with bins, the int32 histograms [P][n_prow][L][B] + the outside count; on the profile rows, keyed like the profile table
    int stor_layers = 0;         // 0: off
    int stor_bins = 0;           // 0: no histogram
    long long stor_grid_y = 65535;   // most member slices of a point in one launch (HYDROCOL_DEBUG_STORAGE_GRID_Y: fewer)
    int stor_range[HC_STORAGE_MAX_LAYERS][2] = {};
    AccTable<long long> stor{"words"};
    AccTable<int> shist{"entries"};
    // ensemble conductivity profiles (hc_set_conductivity_stats): on / off, the layers of K_eff (0: none) and their node
    // ranges; the int64 table kmom [P][n_prow][D][2][5], kcnt [P][n_prow][D][2], kmom_layer [P][n_prow][L][5], kcnt_layer
    // [P][n_prow][L], ovf, on the profile rows and keyed like the profile table; the vector of h->fresh the last launch
    // staged last (-1: none), which is its last row's own when that row refreshed
    bool cond_on = false;
    int cond_layers = 0;
    int cond_range[HC_STORAGE_MAX_LAYERS][2] = {};
    AccTable<long long> cond{"words"};
    int64_t cond_fresh_last = -1;
    // ensemble covariance of theta(z) and the water table (hc_set_theta_cov): the node stride; the int64 table
    // [P][n_prow][W] + the outside word, on the profile rows and keyed like the profile table; the members' quantised rows
    // uint32 [P][chunk][E64], allocated by the first launch; HYDROCOL_COV_CHUNK_MEMBERS (0: from COV_Q_BYTES)
    int cov_stride = 0;          // 0: off
    AccTable<long long> cov{"words"};
    DevBuf<unsigned> cov_q;
    long long cov_chunk = 0;
    // period totals per member (hc_set_period_totals): the periods' inclusive end rows, the threshold nodes, the flux
    // histograms' bin count and range exponents; the members' int64 accumulators [K][N] keyed by (N, K) and their second
    // buffer for the particle filter's ancestry; the int64 table pmom [P][n_period][K][5], pcnt, ovf and, with bins, the
    // int32 table phist_flux [P][n_period][2][B], phist_wtd [P][n_period][2][D] + the outside count, keyed like the profile table
    int per_n = 0;               // 0: off
    std::vector<int64_t> per_end;
    int per_nthr = 0, per_bins = 0;
    int per_thr[HC_PERIOD_MAX_THRESHOLDS] = {};
    int per_fexp[2] = {};
    AccTable<long long> pacc{"words"};
    DevBuf<long long> pacc_alt;
    AccTable<long long> pmom{"words"};
    AccTable<int> phist{"entries"};
    // root-water uptake by depth (hc_set_root_uptake), on the period totals' periods: the layers' midpoint-cell ranges and
    // the share histograms' bin count; the points' midpoint tables as hc_set_column / hc_add_point received them plus
    // 1 / (por - wlt), [P][5][D - 1], on the host and (uploaded by the first call that needs them) on the device; the
    // members' int64 accumulators [L + 1][N] keyed by (N, L + 1) and their second buffer for the particle filter's
    // ancestry; the int64 table umom [P][n_period][L + 1][5], ucnt, uprof [P][n_period][D - 1][2], ovf and, with bins, the
    // int32 table [P][n_period][L][B] + the outside count, keyed like the profile table; the forcing's daylight on the host
    int upt_layers = 0;          // 0: off
    int upt_bins = 0;            // 0: no histogram
    int upt_range[HC_UPTAKE_MAX_LAYERS][2] = {};
    std::vector<double> mid_host;
    DevBuf<double> mid_tabs;
    bool mid_dirty = true;
    AccTable<long long> uacc{"words"};
    DevBuf<long long> uacc_alt;
    AccTable<long long> upt{"words"};
    AccTable<int> uhist{"entries"};
    std::vector<unsigned char> h_daylight;
    // particle filter on the well's water table (hc_set_filter): diagnostics float64 [P][n_arow][4] keyed by
    // (points, rows, stride), the second state / base buffers of the gather, the last assimilation's q_b, {Q, r} and
    // ancestors (test hooks), and the host copy of wtd_obs that decides which rows are assimilated
    int filt_stride = 0;         // 0: off
    double filt_sigma = 0.0;
    uint64_t filt_seed = 0;
    bool filt_done = false;      // an assimilation has run since the filter was set
    bool filt_host() const { return filt_stride > 0 && philox; }   // Philox noise handed to the kernel as caller noise
    AccTable<double> filt{"entries"};
    DevBuf<double> psi_alt, base_alt;
    DevBuf<long long> filt_q, filt_anc, filt_tiles, filt_rows;
    DevBuf<unsigned long long> filt_qr, filt_surv;
    std::vector<long long> filt_rows_host;
    std::vector<int> h_wtd_obs;
    // soil-moisture sensors in the particle filter (hc_set_filter_soil_moisture): the record.  Per member (the last
    // assimilation: test hooks) the weight q_m and the row (l_m, theta of the present sensors, exp(l_m - s)); per point
    // and tile of FILT_TILE members the largest l_m, the integer sums (Q, sum q^2 in two words, count) and the partials
    // of the column sums; per point s and the columns' sums and means
    SmRecord filt_sm;
    DevBuf<long long> filt_qm;
    DevBuf<double> filt_Y, filt_lmax, filt_part, filt_sums;
    DevBuf<unsigned long long> filt_ipart;
    // tempered weights (hc_set_filter_tempering): the ESS floor (0: off); the table float64 [P][n_arow][4] keyed like the
    // filter's; the last assimilation's trials [P][11][4] (test hook); on a sensor row every point's search state and the
    // tiles' integer sums of one trial
    double filt_floor = 0.0;
    AccTable<double> ftemp{"entries"};
    DevBuf<long long> filt_trials, filt_tstate;
    DevBuf<unsigned long long> filt_tpart;
    // rejuvenated base vectors (hc_set_filter_rejuvenation): the discount (0: off) and the shrinkage a, h; the table
    // float64 [P][n_arow][4] keyed like the filter's; the spread passes' tile partials [P][tiles][D] and sums [2][P][D];
    // the last row's moments [P][3][D] (test hook) and refused counts [P]
    double rj_delta = 0.0, rj_a = 0.0, rj_h = 0.0;
    AccTable<double> frej{"entries"};
    DevBuf<double> rj_part, rj_sums, rj_mom;
    DevBuf<unsigned long long> rj_refused;
    // the well's record inside the window (hc_set_filter_window): the window, of each member's water-table index on the
    // lagged rows; per member the largest of its indices on a windowed row (what counts it).  filt_ycols = the width
    // of Y on the last assimilation, m_s + m_w + 2 (0: it took the bin path)
    Window<int> filt_win;
    DevBuf<unsigned short> fwin_wmax;
    int filt_ycols = 0;
    // one point's members on several handles (hc_set_filter_shard): the shard count (0: off), this handle's index and the
    // bounds b_0 = 0 < ... < b_S = n_global, on the host and on the device; the caller's buffer -- the gathered
    // water-table indices [n_global], the send region [(n + S - 1) 2 D] and the receive region [n 2 D], in 8-byte
    // words -- and callbacks; the gathered indices narrowed for the ancestry kernels, every slot's rank among the
    // distinct ancestors, the routing table [6][S] (received / sent members per shard, their offsets in the regions,
    // the first slot of each run), the members to pack and every slot's source
    int fs_n = 0, fs_index = 0;
    std::vector<long long> fs_bounds;
    int64_t fs_words = 0;
    long long *fs_buf = nullptr;
    hc_enkf_exchange_fn fs_gather = nullptr;
    hc_filter_route_fn fs_route = nullptr;
    void *fs_ctx = nullptr;
    DevBuf<long long> fs_bounds_dev, fs_rank, fs_table, fs_list, fs_src;
    DevBuf<unsigned short> fs_w;
    std::vector<long long> fs_counts;
    std::vector<int64_t> fs_send_words, fs_recv_words;
    // fixed-lag smoother of the water table by ancestry (hc_set_filter_smoother): the stride (0: off) and the lag K in
    // record rows; the ring of K + 1 planes -- the members' water-table indices uint16 [K + 1][N], the index within its
    // point of the member each slot descends from uint32 [K + 1][N], their second buffers for the ancestry, and on the
    // host the forcing row each plane holds (-1: none); the last row stepped (what a flush conditions on; -1: none);
    // the tables shist int32 [P][n_srow][D] and spaths int64 [P][n_srow][2], keyed by (points, rows, depth)
    int smo_stride = 0, smo_lag = 0;
    DevBuf<unsigned short> smo_w, smo_w_alt;
    DevBuf<unsigned> smo_id, smo_id_alt;
    std::vector<int64_t> smo_row;
    int64_t smo_last = -1;
    AccTable<int> smo_hist{"entries"};
    AccTable<long long> smo_paths{"entries"};
    // ensemble Kalman filter (hc_set_enkf): diagnostics float64 [P][n_arow][8] keyed by (points, rows, stride); per
    // member the observations Y [N][m'] (the well's y first), the well's eps, the sensors' eps [N][n_s] and the
    // posterior (y, theta..., rejected); what the analysis keeps of psi (EnkfVec, the spread only when psi is relaxed; the
    // posterior's passes over Ypost reuse s1 and s2, so s2 holds the wider of the two); every pass's tile partials
    int enkf_stride = 0;         // 0: off
    double enkf_sigma = 0.0, enkf_loc = 0.0;
    uint64_t enkf_seed = 0;
    bool enkf_done = false;      // an analysis has run since the EnKF was set
    int enkf_width = 0;          // its m' (the rows of Y and the gain)
    AccTable<double> enkf{"entries"};
    DevBuf<double> enkf_Y, enkf_eps, enkf_eps_s, enkf_Ypost, enkf_part, enkf_part_sq;
    EnkfVec enkf_psi;
    // the analysis scheme (hc_set_enkf_method): 0 = perturbed observations, 1 = square root; relaxation of psi to prior
    // spread alpha; what the last analysis ran with
    int enkf_method = 0, enkf_last_method = 0;
    double enkf_alpha = 0.0;
    bool enkf_last_relaxed = false;
    // soil-moisture sensors in the EnKF analysis (hc_set_enkf_soil_moisture): the record
    SmRecord enkf_sm;
    // the well's record inside the window (hc_set_enkf_window): the window, of each member's y on the lagged rows; the
    // last analysis's draws [N][m_w]
    Window<double> enkf_win;
    DevBuf<double> enkf_eps_w;
    // one point's members on several handles (hc_set_enkf_shard): the point's member count (0: off) and this handle's
    // first member in it; the caller's exchange buffer and callback; the point's first member's analysis column [D]
    int64_t shard_global = 0, shard_first = 0, shard_words = 0;
    double *shard_buf = nullptr;
    hc_enkf_exchange_fn shard_fn = nullptr;
    void *shard_ctx = nullptr;
    DevBuf<double> enkf_first;
    // the members' base noise vectors in the analysis (hc_set_enkf_noise_field): on / off and the relaxation of their
    // anomalies; diagnostics float64 [P][n_arow][4 D + 1] keyed like the EnKF's; what the analysis keeps of z (EnkfVec,
    // always with the spread: the table reports it); per member whether its vector was refused, and the count per point
    bool enkf_nz = false, nz_done = false;   // on; an analysis has updated the vectors since it was set
    double enkf_nz_alpha = 0.0;
    // filt_host(), the noise field's twin, or a correlated Philox source
    bool noise_host() const { return (filt_stride > 0 || enkf_nz || ncorr) && philox; }
    AccTable<double> enkf_nzt{"entries"};
    EnkfVec enkf_z;
    DevBuf<double> nz_rej, nz_rejsum;
    // vertical correlation of the Philox source's vectors (hc_set_noise_correlation): on / off, the recursion's
    // coefficients a then b, [2][P][D], on the host and on the device
    bool ncorr = false;
    bool corr_host() const { return ncorr && philox && filt_stride <= 0 && !enkf_nz; }   // ... and nothing else owns base
    std::vector<double> ncorr_ab;
    DevBuf<double> ncorr_dev;
    // perturbed forcing (hc_set_forcing_perturbation): on / off and the parameters; the carried state g [2][N], its second
    // buffer for the particle filter's ancestry and the day it stands at (-1: none yet); the factors of one launch's days
    bool fp_on = false;
    double fp_sigma[2] = {}, fp_phi = 0.0, fp_c = 1.0;
    uint64_t fp_seed = 0;
    int64_t fp_day = -1;
    int64_t fp_day_next = -1;    // the day fp_g_alt stands at: a fill is pending until its step launch is issued
    int64_t fp_offset = -1;      // hc_set_forcing_member_offset (-1: the noise source's)
    DevBuf<double> fp_g, fp_g_alt, fp_fmul;
    // the members' forcing state in the EnKF analysis (hc_set_enkf_forcing): on / off and the relaxation of its anomalies;
    // diagnostics float64 [P][n_arow][9] keyed like the EnKF's; g as the member-major columns x [N][2] the analysis
    // works on; what it keeps of x (EnkfVec with D = 2, always with the spread); the refused members and their count
    bool enkf_fg = false, fg_done = false;   // on; an analysis has updated g since it was set
    double enkf_fg_alpha = 0.0;
    AccTable<double> enkf_fgt{"entries"};
    EnkfVec enkf_gv;
    DevBuf<double> fg_x, fg_rej, fg_rejsum;
    int n_cu = 256;
    double jac_reject = NUM_JAC_DIFF_REJECT;
};

// ------------------------------------------------------------------ auxiliary kernels
namespace hc {

// per-row ensemble moments of the water-table index: one block per row, single writer
// (blockIdx.y = parameter point: its members are contiguous, its table is moments[point][3][n_forcing])
__global__ void moments_kernel(const unsigned short *wtd, const int *wtd_obs, long long n_members,
                               long long members_per_point, long long row_begin, long long n_forcing,
                               long long *moments_all)
{
    const int r = blockIdx.x;
    const long long row = row_begin + r;
    const long long first = (long long)blockIdx.y * members_per_point;
    long long *moments = moments_all + (size_t)blockIdx.y * 3 * n_forcing;
    long long s1 = 0, s2 = 0;
    for (long long k = first + threadIdx.x; k < first + members_per_point; k += blockDim.x) {
        const long long w = wtd[(size_t)r * n_members + k];
        s1 += w;
        s2 += w * w;
    }
    __shared__ long long sh1[256], sh2[256];
    sh1[threadIdx.x] = s1;
    sh2[threadIdx.x] = s2;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh1[threadIdx.x] += sh1[threadIdx.x + o];
            sh2[threadIdx.x] += sh2[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && wtd_obs[row] >= 0) {
        moments[row] += members_per_point;
        moments[n_forcing + row] += sh1[0];
        moments[2 * n_forcing + row] += sh2[0];
    }
}

// ---- ensemble profile statistics (hc_set_profile_stats, include/hydrocol.h): integer sums only
// q = rint(x * 2^s), clamped to |q| <= HC_PROF_Q_MAX (and counted); a member adds q to word 0 and the four 20-bit limbs of
// q^2 (< 2^80) to words 1..4.  Every update is an integer add, so the tables do not depend on launch length, member
// slicing, point order or the number of handles / ranks that are summed.
__device__ __forceinline__ long long prof_quantise(double x, double scale, unsigned &ovf)
{
    double y = rint(x * scale);              // x * 2^s is exact: the rounding is rint's alone
    const double qmax = (double)HC_PROF_Q_MAX;
    if (!(fabs(y) <= qmax)) {                // out of range, infinite or NaN
        ovf++;
        y = (y != y) ? 0.0 : copysign(qmax, y);
    }
    return (long long)y;
}
__device__ __forceinline__ void prof_add(long long (&acc)[HC_PROF_WORDS], long long q)
{
    const unsigned long long a = (unsigned long long)(q < 0 ? -q : q), M = (1ull << 20) - 1;
    const unsigned long long lo = a * a, hi = __umul64hi(a, a);
    acc[0] += q;
    acc[1] += (long long)(lo & M);
    acc[2] += (long long)((lo >> 20) & M);
    acc[3] += (long long)((lo >> 40) & M);
    acc[4] += (long long)(((lo >> 60) | (hi << 4)) & M);
}
constexpr int PROF_TILE = 64;       // nodes per block: one wave-wide, coalesced row segment of a member's state
constexpr int PROF_WAVES = 4;

// psi and theta of one profile row: grid x = 64-node tiles, y = member slices of one point, z = point.  Wave w of a block
// reads members w, w + 4, ... of its slice, lane = node, so every load is 64 contiguous doubles of one member's row.  theta
// is the cell model's own (model_cell, as model_nodes_kernel calls it; theta has no noise term).  The four waves' partial
// sums meet in LDS; wave 0 adds them to the table with int64 atomics (order-independent).  A skipped row (wtd_obs < 0)
// counts nobody unless the row is a snapshot (hc_profile_snapshot: the state before any solve).
__global__ __launch_bounds__(PROF_TILE * PROF_WAVES) void profile_kernel(
    const StepArgs A, const double *node_tabs, int special, const double *stage, const int *wtd_obs, long long row,
    long long prow, long long n_prow, int snapshot, long long members_per_block, long long *prof, long long *pcnt,
    unsigned long long *ovf_word)
{
    if (!snapshot && wtd_obs[row] < 0) return;
    const int D = A.D;
    const int lane = threadIdx.x % PROF_TILE, wave = threadIdx.x / PROF_TILE;
    const int i = blockIdx.x * PROF_TILE + lane;
    const long long point = blockIdx.z;
    const long long end = (point + 1) * A.members_per_point;
    const long long m0 = point * A.members_per_point + (long long)blockIdx.y * members_per_block;
    const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
    long long acc[2][HC_PROF_WORDS] = {};
    unsigned ovf = 0;
    if (i < D) {
        const ColumnDev P = A.P[point];
        const double *nt = node_tabs + (size_t)point * 3 * D;
        const double por = nt[i], meank = nt[D + i], noisec = nt[2 * D + i];
        const double mk = meank == 0.0 ? 1.0e-7 : meank;
        const double rdelta = 1.0 / (por - P.theta_res), logm = log(mk), invm2 = 1.0 / (mk * mk);
        const double s_psi = ldexp(1.0, HC_PROF_SCALE_PSI), s_theta = ldexp(1.0, HC_PROF_SCALE_THETA);
        for (long long m = m0 + wave; m < m1; m += PROF_WAVES) {
            const double psi = stage[(size_t)m * D + i];
            double th, K, C, kb, pf;
            if (special)
                model_cell<true>(P, psi, por, rdelta, logm, invm2, noisec, 0.0, th, K, C, kb, pf);
            else
                model_cell<false>(P, psi, por, rdelta, logm, invm2, noisec, 0.0, th, K, C, kb, pf);
            prof_add(acc[0], prof_quantise(psi, s_psi, ovf));
            prof_add(acc[1], prof_quantise(th, s_theta, ovf));
        }
    }
    __shared__ long long part[PROF_WAVES][2 * HC_PROF_WORDS][PROF_TILE];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int k = 0; k < HC_PROF_WORDS; k++) part[wave][q * HC_PROF_WORDS + k][lane] = acc[q][k];
    __syncthreads();
    if (wave == 0 && i < D) {
        long long *t = prof + (((size_t)point * n_prow + prow) * D + i) * 2 * HC_PROF_WORDS;
#pragma unroll
        for (int w = 0; w < 2 * HC_PROF_WORDS; w++) {
            long long sum = 0;
#pragma unroll
            for (int v = 0; v < PROF_WAVES; v++) sum += part[v][w][lane];
            atomicAdd(reinterpret_cast<unsigned long long *>(t + w), (unsigned long long)sum);
        }
    }
    if (ovf) atomicAdd(ovf_word, (unsigned long long)ovf);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(pcnt + (size_t)point * n_prow + prow), (unsigned long long)(m1 - m0));
}

// ---- ensemble soil-moisture histograms (hc_set_theta_hist, include/hydrocol.h)
// theta of one profile row, counted per node: profile_kernel's shape (grid x = 64-node tiles, y = member slices of one
// point, z = point; lane = node, wave w reads members w, w + 4, ... of its slice, every load 64 contiguous doubles of one
// member's row) and its theta.  The block counts in LDS, bin-major: uint32 [B][64], word b 64 + lane.  Lane l of a
// ds_add_u32 is then on bank l of its half-wave whatever bins the members fall in, so lanes never share an address or a
// bank (the opposite of wtd_hist_kernel, whose lanes share one address and are grouped by ballot first); only the four
// waves of a block meet, through the LDS atomic.  B = 128 is 32 KiB a block, the most that leaves four or five blocks to
// a CU.  The members of one node sit in a few bins, so after the barrier only the nonzero counters go to the table, with
// int32 atomics (integer adds: order-independent), and the block's outside count with one 64-bit atomic when there is
// any.  Lanes past the column take no part; an empty slice writes nothing.
__global__ __launch_bounds__(PROF_TILE * PROF_WAVES) void theta_hist_kernel(
    const StepArgs A, const double *node_tabs, int special, const double *stage, const int *wtd_obs, long long row,
    long long prow, long long n_prow, int snapshot, long long members_per_block, int B, int *hist,
    unsigned long long *outside_word)
{
    if (!snapshot && wtd_obs[row] < 0) return;
    const int D = A.D;
    const int lane = threadIdx.x % PROF_TILE, wave = threadIdx.x / PROF_TILE;
    const int i = blockIdx.x * PROF_TILE + lane;
    const long long point = blockIdx.z;
    const long long end = (point + 1) * A.members_per_point;
    const long long m0 = point * A.members_per_point + (long long)blockIdx.y * members_per_block;
    const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
    if (m0 >= m1) return;                    // (the whole block: nothing is shared yet)
    extern __shared__ unsigned theta_bins[];     // [B][PROF_TILE]
    __shared__ unsigned outside_sum;
    const int words = B * PROF_TILE;
    for (int k = threadIdx.x; k < words; k += PROF_TILE * PROF_WAVES) theta_bins[k] = 0;
    if (threadIdx.x == 0) outside_sum = 0;
    __syncthreads();
    if (i < D) {
        const ColumnDev P = A.P[point];
        const double *nt = node_tabs + (size_t)point * 3 * D;
        const double por = nt[i], meank = nt[D + i], noisec = nt[2 * D + i];
        const double mk = meank == 0.0 ? 1.0e-7 : meank;
        const double rdelta = 1.0 / (por - P.theta_res), logm = log(mk), invm2 = 1.0 / (mk * mk);
        const double nb = (double)B;
        unsigned outside = 0;
        for (long long m = m0 + wave; m < m1; m += PROF_WAVES) {
            const double psi = stage[(size_t)m * D + i];
            double th, K, C, kb, pf;
            if (special)
                model_cell<true>(P, psi, por, rdelta, logm, invm2, noisec, 0.0, th, K, C, kb, pf);
            else
                model_cell<false>(P, psi, por, rdelta, logm, invm2, noisec, 0.0, th, K, C, kb, pf);
            if (th >= 0.0 && th <= 1.0) {    // (false for a NaN)
                const int b = th == 1.0 ? B - 1 : (int)(th * nb);      // theta B is exact: B is a power of two
                atomicAdd(&theta_bins[b * PROF_TILE + lane], 1u);
            } else {
                outside++;
            }
        }
        if (outside) atomicAdd(&outside_sum, outside);
    }
    __syncthreads();
    int *t = hist + ((size_t)point * n_prow + prow) * D * B;
    for (int k = threadIdx.x; k < words; k += PROF_TILE * PROF_WAVES) {
        const unsigned c = theta_bins[k];
        const int node = blockIdx.x * PROF_TILE + k % PROF_TILE;
        if (c && node < D) atomicAdd(t + (size_t)node * B + k / PROF_TILE, (int)c);
    }
    if (threadIdx.x == 0 && outside_sum) atomicAdd(outside_word, (unsigned long long)outside_sum);
}

// ---- ensemble covariance of theta(z) and the water table (hc_set_theta_cov, include/hydrocol.h)
constexpr int COV_TILE = 64;         // columns of a tile, and members of a chunk staged in LDS
constexpr int COV_SLOTS = HC_MAX_DEPTH_NODES / COV_TILE + 1;     // 64-column slots of the widest row (E <= 641)
constexpr int COV_THREADS = 256;

// One profile row's members quantised: layer_storage_kernel's transposed shape.  Grid y = slices of members_per_block
// members of the chunk [c0, c1) of one point's members, z = point; wave w of a block takes members m0 + w, m0 + w + 4,
// ... and its lanes stride over the nodes, so every load is 64 contiguous doubles of one member's row.  psi is read on
// all D nodes for the ballot that gives b (enkf_column_y's rule); theta -- which reads one node constant, the porosity,
// kept in LDS as layer_storage_kernel keeps it -- is evaluated on the selected nodes only, lane l of slot c owning column
// c 64 + l.  The wave votes on validity and writes the member's row of Q, uint32 [point][cap][E64]: the pads are zero and
// a member that is not counted gets an all-zero row, so the product kernel needs no mask.  The wave keeps S1 of its
// members in lane-owned registers; per block S1, count and outside meet in LDS and go to the table with integer atomics
// (order-independent).
__global__ __launch_bounds__(PROF_TILE * PROF_WAVES) void theta_cov_quantise_kernel(
    const StepArgs A, const double *node_tabs, int special, const double *stage, const int *wtd_obs, long long row,
    long long prow, long long n_prow, int snapshot, long long members_per_block, long long c0, long long c1, long long cap,
    int s, int n, int E64, long long W, unsigned *Q, long long *cov, unsigned long long *outside_word)
{
#pragma clang fp contract(off)
    if (!snapshot && wtd_obs[row] < 0) return;
    const int D = A.D, E = n + 1;
    const int lane = threadIdx.x % PROF_TILE, wave = threadIdx.x / PROF_TILE;
    const long long point = blockIdx.z;
    const long long m0 = c0 + (long long)blockIdx.y * members_per_block;
    const long long m1 = m0 + members_per_block < c1 ? m0 + members_per_block : c1;
    if (m0 >= m1) return;                    // (the whole block: nothing is shared yet)
    extern __shared__ double cov_por[];      // [D]
    __shared__ unsigned long long s1_sum[COV_SLOTS * COV_TILE];
    __shared__ unsigned counted_sum, outside_sum;
    const ColumnDev P = A.P[point];
    for (int i = threadIdx.x; i < D; i += PROF_TILE * PROF_WAVES) cov_por[i] = node_tabs[(size_t)point * 3 * D + i];
    for (int k = threadIdx.x; k < COV_SLOTS * COV_TILE; k += PROF_TILE * PROF_WAVES) s1_sum[k] = 0;
    if (threadIdx.x == 0) counted_sum = 0, outside_sum = 0;
    __syncthreads();

    unsigned long long s1[COV_SLOTS] = {};   // lane l: the wave's sums of columns c 64 + l
    unsigned counted = 0, outside = 0;
    const double scale = ldexp(1.0, HC_THETA_COV_SCALE);
    for (long long m = m0 + wave; m < m1; m += PROF_WAVES) {
        const double *psi_m = stage + (size_t)(point * A.members_per_point + m) * D;
        int deepest = -1;
        for (int i0 = 0; i0 < D; i0 += PROF_TILE) {
            const int i = i0 + lane;
            const unsigned long long u = __ballot(i < D && !(psi_m[i] >= P.psi_sat));
            if (u) deepest = i0 + 63 - __clzll((long long)u);
        }
        const int b = deepest < 0 ? 0 : (deepest + 1 < D - 1 ? deepest + 1 : D - 1);
        unsigned q[COV_SLOTS];
        bool bad = false;
#pragma unroll
        for (int c = 0; c < COV_SLOTS; c++) {
            const int k = c * COV_TILE + lane;
            q[c] = k == n ? (unsigned)b : 0u;
            if (k < n) {
                const int i = k * s;
                double th, K, C, kb, pf;
                if (special)
                    model_cell<true>(P, psi_m[i], cov_por[i], 0.0, 0.0, 0.0, 0.0, 0.0, th, K, C, kb, pf);
                else
                    model_cell<false>(P, psi_m[i], cov_por[i], 0.0, 0.0, 0.0, 0.0, 0.0, th, K, C, kb, pf);
                const bool ok = th >= 0.0 && th <= 1.0;          // (false for a NaN)
                q[c] = ok ? (unsigned)rint(th * scale) : 0u;      // theta 2^20 is exact: the rounding is rint's alone
                bad = bad || !ok;
            }
        }
        const bool refused = __ballot(bad) != 0;
        unsigned *qrow = Q + ((size_t)point * cap + (size_t)(m - c0)) * E64;
#pragma unroll
        for (int c = 0; c < COV_SLOTS; c++) {
            const int k = c * COV_TILE + lane;
            if (k < E64) {
                const unsigned v = refused ? 0u : q[c];
                qrow[k] = v;
                s1[c] += v;
            }
        }
        if (refused) outside++; else counted++;
    }
#pragma unroll
    for (int c = 0; c < COV_SLOTS; c++)
        if (s1[c]) atomicAdd(&s1_sum[c * COV_TILE + lane], s1[c]);
    if (lane == 0) {
        if (counted) atomicAdd(&counted_sum, counted);
        if (outside) atomicAdd(&outside_sum, outside);
    }
    __syncthreads();
    long long *t = cov + ((size_t)point * n_prow + prow) * W;
    for (int k = threadIdx.x; k < E; k += PROF_TILE * PROF_WAVES) {
        const unsigned long long v = s1_sum[k];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(t + 1 + k), v);
    }
    if (threadIdx.x == 0) {
        if (counted_sum) atomicAdd(reinterpret_cast<unsigned long long *>(t), (unsigned long long)counted_sum);
        if (outside_sum) atomicAdd(outside_word, (unsigned long long)outside_sum);
    }
}

// S2 += Q^T Q of one chunk, in integers: grid x = pairs I <= J of 64-column tiles (row-major over the upper triangle), y =
// slices of `slice` members of the chunk's `members`, z = point.  The block stages 64 members of both column tiles in LDS
// as uint32 [member][64] -- 16 KiB each, one array on a diagonal pair -- and thread (ty, tx) of the 16 x 16 owns rows
// 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3 of the 64 x 64 output in sixteen 64-bit accumulators; a product is one
// 32 x 32 -> 64-bit multiply-add.  A member's row of a tile is 256 bytes, the 64 banks of a 16-byte read once: the sixteen
// tx of a read's lane group take its sixteen 16-byte slots (the lanes 16 apart that share one share its address), the ty
// of a group are one address per sixteen lanes on distinct banks, so both reads are conflict-free or broadcast.  After its
// slice the block adds the entries with a <= b < E to the table with 64-bit integer atomics, a diagonal pair its upper
// triangle only; zeros (the pads, columns nobody moved) are skipped.  No floating point: no result depends on the slice
// length or on any order.
__global__ __launch_bounds__(COV_THREADS) void theta_cov_syrk_kernel(
    const int *wtd_obs, long long row, long long prow, long long n_prow, int snapshot, long long members, long long cap,
    long long slice, int E, int E64, long long W, const unsigned *Q, long long *cov)
{
    if (!snapshot && wtd_obs[row] < 0) return;
    const int nt = E64 / COV_TILE;
    int p = blockIdx.x, I = 0;
    while (p >= nt - I) p -= nt - I, I++;
    const int J = I + p;
    const long long point = blockIdx.z;
    const long long ms0 = (long long)blockIdx.y * slice;
    const long long ms1 = ms0 + slice < members ? ms0 + slice : members;
    if (ms0 >= ms1) return;                  // (the whole block: nothing is shared yet)
    __shared__ __attribute__((aligned(16))) unsigned tile_a[COV_TILE][COV_TILE], tile_b[COV_TILE][COV_TILE];
    const unsigned (*rhs)[COV_TILE] = I == J ? tile_a : tile_b;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    unsigned long long acc[4][4] = {};
    const unsigned *Qp = Q + (size_t)point * cap * E64;
    for (long long kc = ms0; kc < ms1; kc += COV_TILE) {
#pragma unroll
        for (int j = 0; j < COV_TILE * COV_TILE / 4 / COV_THREADS; j++) {
            const int idx = threadIdx.x + COV_THREADS * j, mm = idx / 16, c4 = idx % 16;
            const long long m = kc + mm;
            uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
            if (m < ms1) {
                const unsigned *r = Qp + (size_t)m * E64;
                a = *reinterpret_cast<const uint4 *>(r + COV_TILE * I + 4 * c4);
                if (I != J) b = *reinterpret_cast<const uint4 *>(r + COV_TILE * J + 4 * c4);
            }
            *reinterpret_cast<uint4 *>(&tile_a[mm][4 * c4]) = a;
            if (I != J) *reinterpret_cast<uint4 *>(&tile_b[mm][4 * c4]) = b;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < COV_TILE; k++) {
            const uint4 a = *reinterpret_cast<const uint4 *>(&tile_a[k][4 * ty]);
            const uint4 b = *reinterpret_cast<const uint4 *>(&rhs[k][4 * tx]);
            const unsigned av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] += (unsigned long long)av[r] * bv[c];
        }
        __syncthreads();
    }
    long long *S2 = cov + ((size_t)point * n_prow + prow) * W + 1 + E;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const long long a = COV_TILE * I + 4 * ty + r;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const long long b = COV_TILE * J + 4 * tx + c;
            if (a <= b && b < E && acc[r][c])
                atomicAdd(reinterpret_cast<unsigned long long *>(S2 + a * E - a * (a - 1) / 2 + (b - a)), acc[r][c]);
        }
    }
}

// ---- ensemble soil-water storage by depth layer (hc_set_layer_storage, include/hydrocol.h)
// the layers of a handle as a kernel argument: node ranges [i0, i1), and [lo, hi) = the nodes any layer holds
struct StorLayers {
    int n, lo, hi;
    int i0[HC_STORAGE_MAX_LAYERS], i1[HC_STORAGE_MAX_LAYERS];
};

// One profile row's storage per member and layer: the transpose of profile_kernel.  Grid y = member slices of one point
// (block y takes slices y, y + gridDim.y, ...: the grid is capped, a point of any size is served), z = point; wave w of a
// block takes members m0 + w, m0 + w + 4, ... of a slice and its lanes stride over the nodes, so every load is 64
// contiguous doubles of one member's row (only the nodes some layer holds are read).  theta reads one node constant, the
// porosity (model_cell's inv_delta is unused, logm, invm2, noisec and the noise feed K_bkg alone, which is dead code
// here as in profile_kernel): the block keeps por [D] in LDS, read with lane = consecutive double, and hands model_cell
// zeros for the rest.  Lane j adds theta_i, i mod 64 == j ascending, into one accumulator per
// layer; a node outside the layer adds 0.0, which leaves an accumulator that started at 0.0 as it is, bit for bit (it is
// never -0.0).  The 64 lane sums meet by halving strides; lane 0's is T (the order of include/hydrocol.h).  Lane l then
// owns layer l: it quantises S = dz T and keeps the wave's five words in registers, and adds one to bin floor(u B) of the
// block's LDS histogram, uint32 [L][B] -- one LDS add per wave, member and layer, on the lanes' own addresses; two waves
// meet on a bin only through the LDS atomic.  After the barrier L x 5 threads add the four waves' words to the table and
// the nonzero bins go to the histogram, all with integer atomics (order-independent); no floating-point atomic anywhere.
__global__ __launch_bounds__(PROF_TILE * PROF_WAVES) void layer_storage_kernel(
    const StepArgs A, const double *node_tabs, int special, const double *stage, const int *wtd_obs, long long row,
    long long prow, long long n_prow, int snapshot, long long members_per_block, const StorLayers Ly, int B,
    long long *stor, long long *scnt, unsigned long long *ovf_word, int *hist, unsigned long long *outside_word)
{
#pragma clang fp contract(off)
    if (!snapshot && wtd_obs[row] < 0) return;
    const int D = A.D, L = Ly.n;
    const int lane = threadIdx.x % PROF_TILE, wave = threadIdx.x / PROF_TILE;
    const long long point = blockIdx.z;
    const long long end = (point + 1) * A.members_per_point;
    const long long slice0 = point * A.members_per_point + (long long)blockIdx.y * members_per_block;
    const long long hop = (long long)gridDim.y * members_per_block;      // to the block's next slice
    if (slice0 >= end) return;               // (the whole block: nothing is shared yet)
    extern __shared__ double stor_lds[];     // por [D], then the bins uint32 [L][B]
    double *por = stor_lds;
    unsigned *bins = reinterpret_cast<unsigned *>(stor_lds + D);
    __shared__ long long part[PROF_WAVES][HC_STORAGE_MAX_LAYERS][HC_PROF_WORDS];
    __shared__ unsigned outside_sum, ovf_sum;
    const ColumnDev P = A.P[point];
    for (int i = Ly.lo + (int)threadIdx.x; i < Ly.hi; i += PROF_TILE * PROF_WAVES) por[i] = node_tabs[(size_t)point * 3 * D + i];
    for (int k = threadIdx.x; k < L * B; k += PROF_TILE * PROF_WAVES) bins[k] = 0;
    if (threadIdx.x == 0) outside_sum = 0, ovf_sum = 0;
    __syncthreads();

    long long words[HC_PROF_WORDS] = {};     // lane l < L: the wave's sums of layer l
    unsigned ovf = 0, outside = 0;
    int own_n = 1;                           // nodes of the lane's own layer (selects: a kernel argument is not indexed by the lane)
#pragma unroll
    for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++) own_n = (lane == l && l < L) ? Ly.i1[l] - Ly.i0[l] : own_n;
    const double s_stor = ldexp(1.0, HC_PROF_SCALE_STORAGE), dz = P.dz, nb = (double)B;
    const int first = Ly.lo / PROF_TILE * PROF_TILE + lane;      // lane j takes nodes i mod 64 == j
    long long counted = 0;                   // members of the block's slices
    for (long long m0 = slice0; m0 < end; m0 += hop) {
        const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
        counted += m1 - m0;
        for (long long m = m0 + wave; m < m1; m += PROF_WAVES) {
            const double *psi_m = stage + (size_t)m * D;
            double x[HC_STORAGE_MAX_LAYERS];
#pragma unroll
            for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++) x[l] = 0.0;
            for (int i = first; i < Ly.hi; i += PROF_TILE) {
                if (i < Ly.lo) continue;
                double th, K, C, kb, pf;
                if (special)
                    model_cell<true>(P, psi_m[i], por[i], 0.0, 0.0, 0.0, 0.0, 0.0, th, K, C, kb, pf);
                else
                    model_cell<false>(P, psi_m[i], por[i], 0.0, 0.0, 0.0, 0.0, 0.0, th, K, C, kb, pf);
#pragma unroll
                for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++)
                    if (l < L) x[l] += (i >= Ly.i0[l] && i < Ly.i1[l]) ? th : 0.0;
            }
            double T = 0.0;
#pragma unroll
            for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++) {
                if (l < L) {                     // (wave-uniform)
                    double v = x[l];
#pragma unroll
                    for (int s = PROF_TILE / 2; s > 0; s >>= 1) v += __shfl_down(v, s, PROF_TILE);
                    const double t = __shfl(v, 0, PROF_TILE);
                    T = lane == l ? t : T;
                }
            }
            if (lane < L) {
                prof_add(words, prof_quantise(dz * T, s_stor, ovf));
                if (B > 0) {
                    const double u = T / (double)own_n;
                    if (u >= 0.0 && u <= 1.0) {      // (false for a NaN)
                        const int b = u == 1.0 ? B - 1 : (int)(u * nb);    // u B is exact: B is a power of two
                        atomicAdd(&bins[lane * B + b], 1u);
                    } else {
                        outside++;
                    }
                }
            }
        }
    }
    if (lane < L) {
#pragma unroll
        for (int k = 0; k < HC_PROF_WORDS; k++) part[wave][lane][k] = words[k];
        if (ovf) atomicAdd(&ovf_sum, ovf);
        if (outside) atomicAdd(&outside_sum, outside);
    }
    __syncthreads();
    if ((int)threadIdx.x < L * HC_PROF_WORDS) {
        const int l = threadIdx.x / HC_PROF_WORDS, k = threadIdx.x % HC_PROF_WORDS;
        long long sum = 0;
#pragma unroll
        for (int v = 0; v < PROF_WAVES; v++) sum += part[v][l][k];
        atomicAdd(reinterpret_cast<unsigned long long *>(stor + (((size_t)point * n_prow + prow) * L + l) * HC_PROF_WORDS + k),
                  (unsigned long long)sum);
    }
    if (B > 0) {
        int *t = hist + ((size_t)point * n_prow + prow) * L * B;
        for (int k = threadIdx.x; k < L * B; k += PROF_TILE * PROF_WAVES) {
            const unsigned c = bins[k];
            if (c) atomicAdd(t + k, (int)c);
        }
    }
    if (threadIdx.x == 0) {
        atomicAdd(reinterpret_cast<unsigned long long *>(scnt + (size_t)point * n_prow + prow), (unsigned long long)counted);
        if (ovf_sum) atomicAdd(ovf_word, (unsigned long long)ovf_sum);
        if (B > 0 && outside_sum) atomicAdd(outside_word, (unsigned long long)outside_sum);
    }
}

// ---- ensemble conductivity profiles (hc_set_conductivity_stats, include/hydrocol.h)
// Where a profile row's noise vector comes from (the rule of include/hydrocol.h), as a kernel argument.  mode: 0 = the
// members' base vectors in memory, 1 = the row's own vectors in memory (`vec` [N][D] in both), 2 = the Philox base (draw 0
// times the member's scale, one product), 3 = the Philox draw of a refresh row.  A refresh row's vector (modes 1, 3) is
// then multiplied by 0.8 once per failed attempt of the row, stats [N][6] being the row's (NULL: no failed attempt).
struct CondNoise {
    int mode;
    const double *vec, *nscale;
    const int *stats;
    unsigned long long seed;
    long long member_offset;
    const long long *point_base;     // NULL with one point
    const int *draw_idx;             // the forcing's draw indices, read at `row` (mode 3)
    long long row;
};
__device__ __forceinline__ double cond_noise(const CondNoise &Z, long long m, long long point, long long members_per_point,
                                             int i, int D)
{
#pragma clang fp contract(off)
    double z;
    if (Z.mode <= 1) {
        z = Z.vec[(size_t)m * D + i];
    } else {
        const long long gid = Z.point_base ? Z.point_base[point] + (m - point * members_per_point) : Z.member_offset + m;
        const unsigned draw = Z.mode == 3 ? (unsigned)Z.draw_idx[Z.row] : 0u;
        z = philox_normal(Z.seed, (unsigned long long)gid, draw, (unsigned)i);
        if (Z.mode == 2) z = z * Z.nscale[m];
    }
    if ((Z.mode & 1) && Z.stats) {
        const int failed = Z.stats[(size_t)m * 6 + 5] >> 8;
        for (int k = 0; k < failed; k++) z = z * 0.8;
    }
    return z;
}
// K_hrc and K_bkg of one node as model_nodes_kernel computes them: the same call on the same values
__device__ __forceinline__ void cond_cell(const ColumnDev &P, int special, double psi, double por, double rdelta, double logm,
                                          double invm2, double noisec, double z, double &K, double &kb)
{
    double th, C, pf;
    if (special)
        model_cell<true>(P, psi, por, rdelta, logm, invm2, noisec, noisec * z, th, K, C, kb, pf);
    else
        model_cell<false>(P, psi, por, rdelta, logm, invm2, noisec, noisec * z, th, K, C, kb, pf);
}
__device__ __forceinline__ bool cond_counted(double K) { return K > 0.0 && K < INFINITY; }      // (false for a NaN)

// ln K_hrc and ln K_bkg of one profile row: profile_kernel's shape (grid x = 64-node tiles, y = member slices of one
// point, z = point; lane = node, wave w reads members w, w + 4, ... of its slice, every psi, base or fresh load 64
// contiguous doubles of one member's row).  A K that is not finite and > 0 adds to no sum: each (node, quantity) keeps its
// own count of the members added.  The four waves' integer partials meet in LDS; wave 0 adds them to the table with int64
// atomics (order-independent).  A skipped row (wtd_obs < 0) counts nobody unless the row is a snapshot.  `eval` (the test
// hook): [4][N][D] = K_hrc, K_bkg, ln K_hrc, ln K_bkg of every member instead, and no table.
__global__ __launch_bounds__(PROF_TILE * PROF_WAVES) void conductivity_kernel(
    const StepArgs A, const double *node_tabs, int special, const double *stage, const int *wtd_obs, long long row,
    long long prow, long long n_prow, int snapshot, long long members_per_block, const CondNoise Z, long long *kmom,
    long long *kcnt, unsigned long long *ovf_word, double *eval)
{
    if (!eval && !snapshot && wtd_obs[row] < 0) return;
    const int D = A.D;
    const int lane = threadIdx.x % PROF_TILE, wave = threadIdx.x / PROF_TILE;
    const int i = blockIdx.x * PROF_TILE + lane;
    const long long point = blockIdx.z;
    const long long end = (point + 1) * A.members_per_point;
    const long long m0 = point * A.members_per_point + (long long)blockIdx.y * members_per_block;
    const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
    long long acc[2][HC_PROF_WORDS] = {};
    long long cnt[2] = {};
    unsigned ovf = 0;
    if (i < D) {
        const ColumnDev P = A.P[point];
        const double *nt = node_tabs + (size_t)point * 3 * D;
        const double por = nt[i], meank = nt[D + i], noisec = nt[2 * D + i];
        const double mk = meank == 0.0 ? 1.0e-7 : meank;
        const double rdelta = 1.0 / (por - P.theta_res), logm = log(mk), invm2 = 1.0 / (mk * mk);
        const double s_lnk = ldexp(1.0, HC_PROF_SCALE_LNK);
        const size_t total = (size_t)A.n_members * D;
        for (long long m = m0 + wave; m < m1; m += PROF_WAVES) {
            const double psi = stage[(size_t)m * D + i];
            const double z = cond_noise(Z, m, point, A.members_per_point, i, D);
            double K[2];
            cond_cell(P, special, psi, por, rdelta, logm, invm2, noisec, z, K[0], K[1]);
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const double lnk = log(K[q]);
                if (eval) {
                    eval[q * total + (size_t)m * D + i] = K[q];
                    eval[(2 + q) * total + (size_t)m * D + i] = lnk;
                } else if (cond_counted(K[q])) {
                    prof_add(acc[q], prof_quantise(lnk, s_lnk, ovf));
                    cnt[q]++;
                }
            }
        }
    }
    if (eval) return;                        // (the whole grid: nothing is shared)
    constexpr int W = 2 * HC_PROF_WORDS + 2;
    __shared__ long long part[PROF_WAVES][W][PROF_TILE];
#pragma unroll
    for (int q = 0; q < 2; q++) {
#pragma unroll
        for (int k = 0; k < HC_PROF_WORDS; k++) part[wave][q * HC_PROF_WORDS + k][lane] = acc[q][k];
        part[wave][2 * HC_PROF_WORDS + q][lane] = cnt[q];
    }
    __syncthreads();
    if (wave == 0 && i < D) {
        const size_t node = ((size_t)point * n_prow + prow) * D + i;
#pragma unroll
        for (int w = 0; w < W; w++) {
            long long sum = 0;
#pragma unroll
            for (int v = 0; v < PROF_WAVES; v++) sum += part[v][w][lane];
            long long *t = w < 2 * HC_PROF_WORDS ? kmom + node * 2 * HC_PROF_WORDS + w : kcnt + node * 2 + (w - 2 * HC_PROF_WORDS);
            if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(t), (unsigned long long)sum);
        }
    }
    if (ovf) atomicAdd(ovf_word, (unsigned long long)ovf);
}

// The effective vertical conductivity of one profile row per member and layer, K_eff = n / sum_i 1 / K_hrc,i (the harmonic
// mean over the layer's n nodes): layer_storage_kernel's shape (grid y = member slices of one point, block y takes slices
// y, y + gridDim.y, ...; a wave owns a member and its lanes stride over the nodes) and its summation order -- lane j adds
// 1 / K_i, i mod 64 == j ascending, a node outside the layer adds 0.0, then the halving tree; nothing contracted.  The
// reduction over depth comes before the one over members: the nodes of one member covary.  Lane l then owns layer l and adds
// q = rint(ln K_eff 2^30) to the wave's five words; a member whose K_eff is not finite and > 0 (one node with K_hrc = 0
// is enough) is left out of that layer, which the layer's count shows.  Integer atomics only.
__global__ __launch_bounds__(PROF_TILE * PROF_WAVES) void conductivity_layer_kernel(
    const StepArgs A, const double *node_tabs, int special, const double *stage, const int *wtd_obs, long long row,
    long long prow, long long n_prow, int snapshot, long long members_per_block, const StorLayers Ly, const CondNoise Z,
    long long *kmom_layer, long long *kcnt_layer, unsigned long long *ovf_word)
{
#pragma clang fp contract(off)
    if (!snapshot && wtd_obs[row] < 0) return;
    const int D = A.D, L = Ly.n;
    const int lane = threadIdx.x % PROF_TILE, wave = threadIdx.x / PROF_TILE;
    const long long point = blockIdx.z;
    const long long end = (point + 1) * A.members_per_point;
    const long long slice0 = point * A.members_per_point + (long long)blockIdx.y * members_per_block;
    const long long hop = (long long)gridDim.y * members_per_block;      // to the block's next slice
    if (slice0 >= end) return;               // (the whole block: nothing is shared yet)
    extern __shared__ double cond_lds[];     // the point's node tables [3][D]
    __shared__ long long part[PROF_WAVES][HC_STORAGE_MAX_LAYERS][HC_PROF_WORDS + 1];
    __shared__ unsigned ovf_sum;
    const ColumnDev P = A.P[point];
    for (int k = threadIdx.x; k < 3 * D; k += PROF_TILE * PROF_WAVES) cond_lds[k] = node_tabs[(size_t)point * 3 * D + k];
    if (threadIdx.x == 0) ovf_sum = 0;
    __syncthreads();

    long long words[HC_PROF_WORDS] = {}, counted = 0;    // lane l < L: the wave's sums of layer l
    unsigned ovf = 0;
    double own_n = 1.0;                      // nodes of the lane's own layer
#pragma unroll
    for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++) own_n = (lane == l && l < L) ? (double)(Ly.i1[l] - Ly.i0[l]) : own_n;
    const double s_lnk = ldexp(1.0, HC_PROF_SCALE_LNK);
    const int first = Ly.lo / PROF_TILE * PROF_TILE + lane;      // lane j takes nodes i mod 64 == j
    for (long long m0 = slice0; m0 < end; m0 += hop) {
        const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
        for (long long m = m0 + wave; m < m1; m += PROF_WAVES) {
            const double *psi_m = stage + (size_t)m * D;
            double x[HC_STORAGE_MAX_LAYERS];
#pragma unroll
            for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++) x[l] = 0.0;
            for (int i = first; i < Ly.hi; i += PROF_TILE) {
                if (i < Ly.lo) continue;
                const double por = cond_lds[i], meank = cond_lds[D + i], noisec = cond_lds[2 * D + i];
                const double mk = meank == 0.0 ? 1.0e-7 : meank;
                const double z = cond_noise(Z, m, point, A.members_per_point, i, D);
                double K, kb;
                cond_cell(P, special, psi_m[i], por, 1.0 / (por - P.theta_res), log(mk), 1.0 / (mk * mk), noisec, z, K, kb);
                const double r = 1.0 / K;
#pragma unroll
                for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++)
                    if (l < L) x[l] += (i >= Ly.i0[l] && i < Ly.i1[l]) ? r : 0.0;
            }
            double T = 0.0;
#pragma unroll
            for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++) {
                if (l < L) {                     // (wave-uniform)
                    double v = x[l];
#pragma unroll
                    for (int s = PROF_TILE / 2; s > 0; s >>= 1) v += __shfl_down(v, s, PROF_TILE);
                    const double t = __shfl(v, 0, PROF_TILE);
                    T = lane == l ? t : T;
                }
            }
            if (lane < L) {
                const double keff = own_n / T;
                if (cond_counted(keff)) {
                    prof_add(words, prof_quantise(log(keff), s_lnk, ovf));
                    counted++;
                }
            }
        }
    }
    if (lane < L) {
#pragma unroll
        for (int k = 0; k < HC_PROF_WORDS; k++) part[wave][lane][k] = words[k];
        part[wave][lane][HC_PROF_WORDS] = counted;
        if (ovf) atomicAdd(&ovf_sum, ovf);
    }
    __syncthreads();
    if ((int)threadIdx.x < L * (HC_PROF_WORDS + 1)) {
        const int l = threadIdx.x / (HC_PROF_WORDS + 1), k = threadIdx.x % (HC_PROF_WORDS + 1);
        long long sum = 0;
#pragma unroll
        for (int v = 0; v < PROF_WAVES; v++) sum += part[v][l][k];
        const size_t slot = ((size_t)point * n_prow + prow) * L + l;
        long long *t = k < HC_PROF_WORDS ? kmom_layer + slot * HC_PROF_WORDS + k : kcnt_layer + slot;
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(t), (unsigned long long)sum);
    }
    if (threadIdx.x == 0 && ovf_sum) atomicAdd(ovf_word, (unsigned long long)ovf_sum);
}

// ---- root-water uptake by depth (hc_set_root_uptake, include/hydrocol.h)
// the layers of a handle as a kernel argument: midpoint-cell ranges [c0, c1); plane 0 of the totals is every cell
struct UptLayers {
    int n;
    int c0[HC_UPTAKE_MAX_LAYERS], c1[HC_UPTAKE_MAX_LAYERS];
};
constexpr int UPT_TAB_POR = 0, UPT_TAB_FC = 1, UPT_TAB_WLT = 2, UPT_TAB_INVD1 = 3, UPT_TAB_ROOT = 4, UPT_NTAB = 5;

// inclusive scan over the 64 lanes by doubling offsets: at offset o lane l >= o adds lane l - o's value of the step before
__device__ __forceinline__ double upt_scan(double v, int lane)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o < PROF_TILE; o <<= 1) {
        const double w = __shfl_up(v, o, PROF_TILE);
        v = lane >= o ? v + w : v;
    }
    return v;
}
// the 64 lanes' values by halving strides (layer_storage_kernel's order), lane 0's total handed to every lane
__device__ __forceinline__ double upt_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int s = PROF_TILE / 2; s > 0; s >>= 1) v += __shfl_down(v, s, PROF_TILE);
    return __shfl(v, 0, PROF_TILE);
}

// One forcing row's uptake per member: layer_storage_kernel's shape.  Grid y = member slices of one point (block y takes
// slices y, y + gridDim.y, ...), z = point; wave w of a block takes members m0 + w, m0 + w + 4, ... of a slice, and lane j
// of it owns the midpoint cells i = 64 r + j of round r = 0, 1, ...: y_i = 0.5 (psi_i + psi_{i+1}) reads two runs of 64
// contiguous doubles of the member's row.  The five midpoint tables of the point (porosity, field capacity, wilting
// point, 1 / (por - wlt), root density: [5][cells] doubles, read with lane = consecutive double, one 256-byte bank row a
// half-wave, no conflict) sit in LDS, and each wave has a row of `cells` doubles of its own there that holds theta, then
// rho, then x of the member in turn: a lane reads back only what it wrote, so the row needs no barrier.  The cell model
// runs on the cells 0 ... n_root_int alone (on every midpoint for the test hook, which also wants theta below the roots).
// The order of every sum is fixed by n_root_int alone (include/hydrocol.h): lane partials over the rounds ascending, the 64
// partials by halving strides; the cumulative theta by a doubling-offset scan per round plus the carry of the rounds
// before, run twice (once for the total, once for the cells) instead of being stored.  Plain IEEE operations, no
// contraction, no reciprocal shortcuts.  Lane l <= L then owns plane l of the member's totals: it quantises U_l and adds
// it to the member's accumulator -- the member belongs to this wave alone, a plain read-modify-write.  The depth-resolved
// q_i go as two 20-bit limbs into the block's LDS image uint64 [n_root_int + 1][2] with ds_add_u64 on the lane's own two
// addresses (16 bytes a lane: a half-wave's 32 lanes cover two bank rows, two passes an instruction; the four waves meet
// on a word only through the LDS atomic, and a zero adds nothing); after the barrier the nonzero words go to uprof with
// int64 atomics.  Integer adds only beyond the member: the tables do not depend on any order.
__global__ __launch_bounds__(PROF_TILE * PROF_WAVES) void root_uptake_kernel(
    const StepArgs A, const double *mid_tabs, int special, const double *stage, const int *wtd_obs, const double *atm,
    const unsigned char *daylight, long long row, long long period, long long n_period, long long members_per_block,
    const UptLayers Ly, long long *uacc, long long *uprof, unsigned long long *ovf_word, double *theta_out, double *u_out)
{
#pragma clang fp contract(off)
    const bool eval = theta_out != nullptr;
    if (!eval && wtd_obs[row] < 0) return;
    const int D = A.D, M = D - 1, L = Ly.n;
    const int lane = threadIdx.x % PROF_TILE, wave = threadIdx.x / PROF_TILE;
    const long long point = blockIdx.z;
    const long long end = (point + 1) * A.members_per_point;
    const long long slice0 = point * A.members_per_point + (long long)blockIdx.y * members_per_block;
    const long long hop = (long long)gridDim.y * members_per_block;
    if (slice0 >= end) return;               // (the whole block: nothing is shared yet)
    const ColumnDev P = A.P[point];
    const int n_int = P.n_root_int;
    const int n_model = eval ? M : n_int + 1;                    // cells the cell model runs on
    const int rounds = (n_model + PROF_TILE - 1) / PROF_TILE, cells = rounds * PROF_TILE;
    const int n_img = 2 * (n_int + 1);
    extern __shared__ double upt_lds[];      // tables [5][cells], the waves' rows [4][cells], the image uint64 [n_int + 1][2]
    double *tab = upt_lds, *ws = upt_lds + (size_t)(UPT_NTAB + wave) * cells;
    unsigned long long *img = reinterpret_cast<unsigned long long *>(upt_lds + (size_t)(UPT_NTAB + PROF_WAVES) * cells);
    __shared__ unsigned ovf_sum;
    for (int k = threadIdx.x; k < UPT_NTAB * cells; k += PROF_TILE * PROF_WAVES) {
        const int t = k / cells, i = k % cells;
        tab[k] = i < n_model ? mid_tabs[((size_t)point * UPT_NTAB + t) * M + i] : 0.0;
    }
    for (int k = threadIdx.x; k < n_img; k += PROF_TILE * PROF_WAVES) img[k] = 0;
    if (threadIdx.x == 0) ovf_sum = 0;
    __syncthreads();

    const double *t_por = tab + UPT_TAB_POR * cells, *t_fc = tab + UPT_TAB_FC * cells, *t_wlt = tab + UPT_TAB_WLT * cells;
    const double *t_invd1 = tab + UPT_TAB_INVD1 * cells, *t_root = tab + UPT_TAB_ROOT * cells;
    const bool on = P.flag_et && (daylight[row] & 1);            // (the hook is a normal-mode call: never a spin-up solve)
    const double atm_r = atm[row], dz = P.dz;
    const double s_flux = ldexp(1.0, HC_PROF_SCALE_FLUX), s_prof = ldexp(1.0, HC_UPTAKE_SCALE_PROFILE);
    const int r_int = (n_int + 1 + PROF_TILE - 1) / PROF_TILE;   // rounds that hold a root cell
    unsigned ovf = 0;
    for (long long m0 = slice0; m0 < end; m0 += hop) {
        const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
        for (long long m = m0 + wave; m < m1; m += PROF_WAVES) {
            const double *psi_m = stage + (size_t)m * D;
            // theta at the midpoints, and sum (theta - wlt) over the interior root cells 1 ... n_int
            double s_w = 0.0, th0 = 0.0;
            for (int r = 0; r < rounds; r++) {
                const int i = r * PROF_TILE + lane;
                double th = 0.0;
                if (i < n_model) {
                    const double y = 0.5 * (psi_m[i] + psi_m[i + 1]);
                    double K, C, kb, pf;
                    if (special)
                        model_cell<true>(P, y, t_por[i], 0.0, 0.0, 0.0, 0.0, 0.0, th, K, C, kb, pf);
                    else
                        model_cell<false>(P, y, t_por[i], 0.0, 0.0, 0.0, 0.0, 0.0, th, K, C, kb, pf);
                    if (eval) theta_out[(size_t)m * M + i] = th;
                }
                ws[i] = th;
                s_w += (i >= 1 && i <= n_int) ? th - t_wlt[i] : 0.0;
                if (r == 0) th0 = __shfl(th, 0, PROF_TILE);
            }
            // (a) the interior call: cells 1 ... n_int normalised together
            double tr_pot = 0.0;             // 0: no uptake in the interior
            if (on && n_int > 0) {
                const double water_k = upt_sum(s_w) * dz;
                double tot_x = 0.0;
                if (water_k > 0.0) {
                    double carry = 0.0;
                    bool all_one = true;
                    for (int r = 0; r < r_int; r++) {
                        const int i = r * PROF_TILE + lane;
                        const bool in = i >= 1 && i <= n_int;
                        const double sc = upt_scan(in ? ws[i] : 0.0, lane);
                        carry = carry + __shfl(sc, PROF_TILE - 1, PROF_TILE);
                        all_one = all_one && (!in || ws[i] > t_fc[i]);
                    }
                    double total = carry * dz;
                    total = total == 0.0 ? 1.0 : total;
                    const double a2v = __all(all_one) ? 0.1 : 1.0;       // the "roots drowning" guard
                    carry = 0.0;
                    double s_r = 0.0;
                    for (int r = 0; r < r_int; r++) {
                        const int i = r * PROF_TILE + lane;
                        const bool in = i >= 1 && i <= n_int;
                        const double th = ws[i];
                        const double sc = upt_scan(in ? th : 0.0, lane);
                        const double local = (carry + sc) * dz;
                        carry = carry + __shfl(sc, PROF_TILE - 1, PROF_TILE);
                        const double a1 = fmax(th * t_invd1[i], local / total);
                        const double rho = (in && th > t_fc[i]) ? fabs(a1 * a2v) : 0.0;
                        ws[i] = rho;
                        s_r += rho;
                    }
                    double tot = upt_sum(s_r) * dz;
                    tot = tot == 0.0 ? 1.0 : tot;
                    double s_x = 0.0;
                    for (int r = 0; r < r_int; r++) {
                        const int i = r * PROF_TILE + lane;
                        const double x = (ws[i] / tot) * t_root[i];
                        ws[i] = x;
                        s_x += x;
                    }
                    tot_x = upt_sum(s_x) * dz;
                    if (tot_x > 1.0) {
                        s_x = 0.0;
                        for (int r = 0; r < r_int; r++) {
                            const int i = r * PROF_TILE + lane;
                            const double x = ws[i] / tot_x;
                            ws[i] = x;
                            s_x += x;
                        }
                        tot_x = upt_sum(s_x) * dz;
                    }
                    if (tot_x > 0.0) tr_pot = fmin(atm_r, water_k) / tot_x;
                }
            }
            const bool have = tr_pot != 0.0;     // (ws holds x only then; a zero rate gives zeros either way)
            // (b) the first-midpoint call: cell 0 normalised on its own, by every lane alike
            double u0 = 0.0;
            if (on && P.n_root_first > 0) {
                const double water_k = (th0 - t_wlt[0]) * dz;
                if (water_k > 0.0) {
                    const double local = th0 * dz;
                    const double total = local == 0.0 ? 1.0 : local;
                    const double a1 = fmax(th0 * t_invd1[0], local / total);
                    double rho = th0 > t_fc[0] ? fabs(a1 * 0.1) : 0.0;   // one cell: above field capacity it is "all cells"
                    double tot = rho * dz;
                    tot = tot == 0.0 ? 1.0 : tot;
                    double x0 = (rho / tot) * t_root[0];
                    double tot_x = x0 * dz;
                    if (tot_x > 1.0) {
                        x0 = x0 / tot_x;
                        tot_x = x0 * dz;
                    }
                    if (tot_x > 0.0) u0 = (fmin(atm_r, water_k) / tot_x) * x0;
                }
            }
            // the member's u_i: the hook's output, or the layer totals and the depth-resolved limbs
            double x[HC_UPTAKE_MAX_LAYERS + 1];
#pragma unroll
            for (int l = 0; l <= HC_UPTAKE_MAX_LAYERS; l++) x[l] = 0.0;
            for (int r = 0; r < (eval ? rounds : r_int); r++) {
                const int i = r * PROF_TILE + lane;
                double u = (have && i >= 1 && i <= n_int) ? tr_pot * ws[i] : 0.0;
                u = i == 0 ? u0 : u;
                if (eval) {
                    if (i < M) u_out[(size_t)m * M + i] = u;
                    continue;
                }
                x[0] += u;
#pragma unroll
                for (int l = 0; l < HC_UPTAKE_MAX_LAYERS; l++)
                    if (l < L) x[l + 1] += (i >= Ly.c0[l] && i < Ly.c1[l]) ? u : 0.0;
                if (i <= n_int) {
                    const long long q = prof_quantise(u, s_prof, ovf);
                    if (q > 0) {
                        atomicAdd(&img[2 * i], (unsigned long long)(q & ((1LL << 20) - 1)));
                        atomicAdd(&img[2 * i + 1], (unsigned long long)(q >> 20));
                    } else if (q < 0) {          // (u >= 0 by construction: a guard that keeps the limbs unsigned)
                        ovf++;
                    }
                }
            }
            if (eval) continue;
            double T = 0.0;
#pragma unroll
            for (int l = 0; l <= HC_UPTAKE_MAX_LAYERS; l++) {
                if (l <= L) {                    // (wave-uniform)
                    const double t = upt_sum(x[l]);
                    T = lane == l ? t : T;
                }
            }
            if (lane <= L) uacc[(size_t)lane * A.n_members + m] += prof_quantise(dz * T, s_flux, ovf);
        }
    }
    if (eval) return;
    if (ovf) atomicAdd(&ovf_sum, ovf);
    __syncthreads();
    long long *t = uprof + ((size_t)point * n_period + period) * M * 2;
    for (int k = threadIdx.x; k < n_img; k += PROF_TILE * PROF_WAVES) {
        const unsigned long long c = img[k];
        if (c) atomicAdd(reinterpret_cast<unsigned long long *>(t + k), c);
    }
    if (threadIdx.x == 0 && ovf_sum) atomicAdd(ovf_word, (unsigned long long)ovf_sum);
}

// transpiration / lateral flow of every solved row of a launch, the member count and sum |obs - wtd| (abs_error in grid
// steps): one block per (launch row, point) as moments_kernel, partial sums through cross-lane shuffles then LDS, one writer
__global__ __launch_bounds__(256) void flux_stats_kernel(const double *diag, const unsigned short *wtd, const int *wtd_obs,
                                                         long long n_members, long long members_per_point, long long row_begin,
                                                         long long n_forcing, long long *flux, long long *fcnt, long long *aerr,
                                                         unsigned long long *ovf_word)
{
    const long long row = row_begin + blockIdx.x;
    const int obs = wtd_obs[row];
    if (obs < 0) return;
    const long long first = (long long)blockIdx.y * members_per_point;
    const double s_flux = ldexp(1.0, HC_PROF_SCALE_FLUX);
    long long acc[2][HC_PROF_WORDS] = {};
    long long ae = 0;
    unsigned ovf = 0;
    for (long long k = first + threadIdx.x; k < first + members_per_point; k += blockDim.x) {
        const size_t e = (size_t)blockIdx.x * n_members + k;
        prof_add(acc[0], prof_quantise(diag[2 * e + 0], s_flux, ovf));
        prof_add(acc[1], prof_quantise(diag[2 * e + 1], s_flux, ovf));
        const int d = obs - (int)wtd[e];
        ae += d < 0 ? -d : d;
    }
    constexpr int NW = 2 * HC_PROF_WORDS + 1;
    long long v[NW];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int k = 0; k < HC_PROF_WORDS; k++) v[q * HC_PROF_WORDS + k] = acc[q][k];
    v[NW - 1] = ae;
#pragma unroll
    for (int w = 0; w < NW; w++)
        for (int o = WAVE / 2; o > 0; o >>= 1) v[w] += __shfl_xor(v[w], o);
    __shared__ long long part[256 / WAVE][NW];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (lane == 0)
#pragma unroll
        for (int w = 0; w < NW; w++) part[wave][w] = v[w];
    if (ovf) atomicAdd(ovf_word, (unsigned long long)ovf);
    __syncthreads();
    if (threadIdx.x < NW) {
        long long sum = 0;
        for (int u = 0; u < (int)(blockDim.x / WAVE); u++) sum += part[u][threadIdx.x];
        const size_t pr = (size_t)blockIdx.y * n_forcing + row;
        if (threadIdx.x < NW - 1)
            flux[pr * 2 * HC_PROF_WORDS + threadIdx.x] += sum;
        else
            aerr[pr] += sum;
    }
    if (threadIdx.x == 0) fcnt[(size_t)blockIdx.y * n_forcing + row] += members_per_point;
}

// ---- ensemble water-table histograms (hc_set_wtd_hist, include/hydrocol.h)
constexpr int HIST_THREADS = 256;

// The histogram rows of one launch: grid x = (histogram row j of the launch) x (member slice), y = point.  Launch row
// first + j stride is forcing row row0 + first + j stride.  Bins are counted in LDS (D <= 640 uint32).  The members of one
// well sit in a few bins, so a plain ds_add_u32 per lane would serialise on one address: each wave first groups its 64
// members by bin (one ballot per distinct bin: a wave of one bin costs one LDS add instead of 64), and one lane adds the
// group's size.  Only nonzero bins go to the table, with int32 atomics (integer adds: order-independent).
__global__ __launch_bounds__(HIST_THREADS) void wtd_hist_kernel(const unsigned short *wtd, const int *wtd_obs,
                                                                long long n_members, long long members_per_point,
                                                                long long members_per_block, int slices, long long row0,
                                                                int first, int stride, long long n_hrow, int D, int *hist)
{
    const long long j = blockIdx.x / slices;
    const long long slice = blockIdx.x % slices;
    const long long r = first + j * stride;
    const long long row = row0 + r;
    if (wtd_obs[row] < 0) return;
    __shared__ unsigned bins[HC_MAX_DEPTH_NODES];
    for (int b = threadIdx.x; b < D; b += HIST_THREADS) bins[b] = 0;
    __syncthreads();
    const long long point = blockIdx.y;
    const long long end = (point + 1) * members_per_point;
    const long long m0 = point * members_per_point + slice * members_per_block;
    const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
    const unsigned short *w = wtd + (size_t)r * n_members;
    const int lane = threadIdx.x % WAVE;
    // wave-uniform trip count: every lane of a wave runs the ballots of every round
    for (long long k0 = m0 + (threadIdx.x - lane); k0 < m1; k0 += HIST_THREADS) {
        const long long k = k0 + lane;
        const int b = k < m1 ? (int)w[k] : -1;
        unsigned long long pending = __ballot(b >= 0 && b < D);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int v = __builtin_amdgcn_readlane(b, leader);
            const unsigned long long same = __ballot(b == v) & pending;
            if (lane == leader) atomicAdd(&bins[v], (unsigned)__popcll(same));
            pending &= ~same;
        }
    }
    __syncthreads();
    int *t = hist + ((size_t)point * n_hrow + (size_t)(row / stride)) * D;
    for (int b = threadIdx.x; b < D; b += HIST_THREADS) {
        const unsigned c = bins[b];
        if (c) atomicAdd(t + b, (int)c);
    }
}

// ---- period totals per member (hc_set_period_totals, include/hydrocol.h): integers only
constexpr int PERIOD_K = 4 + HC_PERIOD_MAX_THRESHOLDS;     // the accumulators a member carries at most
constexpr int PERIOD_THREADS = 256;
constexpr long long PERIOD_WTD_NONE = 65535;               // wtd_shallowest of a member with no solved row yet
struct PeriodThresholds {
    int n;
    int node[HC_PERIOD_MAX_THRESHOLDS];
};

// The launch's rows [0, rows) (forcing rows row0 ...) added to the members' accumulators acc [K][N]: one thread per
// member.  Per row a wave reads 64 x 16 contiguous bytes of diag [rows][N][2] and 64 x 2 of wtd [rows][N]; the K running
// values stay in registers over the rows, ascending, and the accumulators are read and written once per launch (each
// of the K planes coalesced).  A skipped row (wtd_obs < 0, wave-uniform) adds nothing.
__global__ __launch_bounds__(PERIOD_THREADS) void period_accumulate_kernel(
    const double *diag, const unsigned short *wtd, const int *wtd_obs, long long n_members, long long row0, int rows,
    const PeriodThresholds Th, long long *acc, unsigned long long *ovf_word)
{
    const long long m = (long long)blockIdx.x * PERIOD_THREADS + threadIdx.x;
    if (m >= n_members) return;
    const double s_flux = ldexp(1.0, HC_PROF_SCALE_FLUX);
    long long flux0 = 0, flux1 = 0;
    int lo = (int)PERIOD_WTD_NONE, hi = 0;
    int below[HC_PERIOD_MAX_THRESHOLDS] = {};
    unsigned ovf = 0;
    for (int r = 0; r < rows; r++) {
        if (wtd_obs[row0 + r] < 0) continue;
        const size_t e = (size_t)r * n_members + m;
        const double2 d = reinterpret_cast<const double2 *>(diag)[e];
        const int w = (int)wtd[e];
        flux0 += prof_quantise(d.x, s_flux, ovf);
        flux1 += prof_quantise(d.y, s_flux, ovf);
        lo = w < lo ? w : lo;
        hi = w > hi ? w : hi;
#pragma unroll
        for (int j = 0; j < HC_PERIOD_MAX_THRESHOLDS; j++) below[j] += (j < Th.n && w <= Th.node[j]) ? 1 : 0;
    }
    long long *a = acc + m;
    a[0] += flux0;
    a[n_members] += flux1;
    const long long lo0 = a[2 * n_members], hi0 = a[3 * n_members];
    a[2 * n_members] = lo < lo0 ? lo : lo0;
    a[3 * n_members] = hi > hi0 ? hi : hi0;
#pragma unroll
    for (int j = 0; j < HC_PERIOD_MAX_THRESHOLDS; j++)
        if (j < Th.n) a[(size_t)(4 + j) * n_members] += below[j];
    if (ovf) atomicAdd(ovf_word, (unsigned long long)ovf);
}

// one to bin b of every lane that has one (b >= 0), grouped as wtd_hist_kernel groups them: the members of a point sit in
// a handful of bins, so a ds_add_u32 per lane would serialise on a few addresses; one ballot per distinct bin and one
// lane adds the group's size.  Every lane of the wave calls it.
__device__ __forceinline__ void period_bin_add(unsigned *bins, int b, int lane)
{
    unsigned long long pending = __ballot(b >= 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int v = __builtin_amdgcn_readlane(b, leader);
        const unsigned long long same = __ballot(b == v) & pending;
        if (lane == leader) atomicAdd(&bins[v], (unsigned)__popcll(same));
        pending &= ~same;
    }
}

// The end of period `period`: grid x = member slices of one point, y = point.  A member with a solved row in the period
// (wtd_shallowest != 65535) enters the moments pmom [P][n_period][K][5] -- the flux totals as v = A >> 12 (floor; 2^-20
// cm), clamped to HC_PROF_Q_MAX and counted, indices and counts as they are -- through prof_add in registers, cross-lane
// shuffles, LDS and int64 atomics, and, with B > 0, the block's LDS histograms uint32 [2][B] (bin (v B) >> sh_q of
// 0 <= v < 2^sh_q, sh_q = 20 + e_q; others count as outside) and [2][D] (shallowest, deepest index).  Only nonzero bins
// go to the tables (int32 atomics).  Every member's accumulators are reset.
__global__ __launch_bounds__(PERIOD_THREADS) void period_reduce_kernel(
    long long *acc, long long n_members, long long members_per_point, long long members_per_block, long long period,
    long long n_period, int K, int B, int D, int sh0, int sh1, long long *pmom, long long *pcnt,
    unsigned long long *ovf_word, int *hist_flux, int *hist_wtd, unsigned long long *outside_word)
{
    extern __shared__ unsigned period_bins[];        // flux [2][B], then wtd [2][D]
    __shared__ long long part[PERIOD_THREADS / WAVE][PERIOD_K][HC_PROF_WORDS];
    __shared__ long long cnt_part[PERIOD_THREADS / WAVE];
    __shared__ unsigned ovf_sum, outside_sum;
    const int n_bins = B > 0 ? 2 * (B + D) : 0;
    for (int b = threadIdx.x; b < n_bins; b += PERIOD_THREADS) period_bins[b] = 0;
    if (threadIdx.x == 0) ovf_sum = 0, outside_sum = 0;
    __syncthreads();
    const long long point = blockIdx.y;
    const long long end = (point + 1) * members_per_point;
    const long long m0 = point * members_per_point + (long long)blockIdx.x * members_per_block;
    const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const long long qmax = HC_PROF_Q_MAX;
    long long words[PERIOD_K][HC_PROF_WORDS] = {};
    long long counted = 0;
    unsigned ovf = 0, outside = 0;
    // wave-uniform trip count: every lane of a wave runs the ballots of every round
    for (long long k0 = m0 + (threadIdx.x - lane); k0 < m1; k0 += PERIOD_THREADS) {
        const long long m = k0 + lane;
        const bool live = m < m1;
        long long a[PERIOD_K];
#pragma unroll
        for (int k = 0; k < PERIOD_K; k++) a[k] = (live && k < K) ? acc[(size_t)k * n_members + m] : 0;
        int bin[4] = {-1, -1, -1, -1};
        if (live && a[2] != PERIOD_WTD_NONE) {
            counted++;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                long long v = a[q] >> 12;            // floor(A / 4096)
                if (v > qmax) v = qmax, ovf++;
                if (v < -qmax) v = -qmax, ovf++;
                prof_add(words[q], v);
                if (B > 0) {
                    const int sh = q ? sh1 : sh0;
                    if (v >= 0 && v < (1LL << sh))
                        bin[q] = q * B + (int)((v * B) >> sh);
                    else
                        outside++;
                }
            }
#pragma unroll
            for (int k = 2; k < PERIOD_K; k++)
                if (k < K) prof_add(words[k], a[k]);
            if (B > 0) {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    if (a[2 + q] >= 0 && a[2 + q] < D)
                        bin[2 + q] = 2 * B + q * D + (int)a[2 + q];
                    else
                        outside++;
                }
            }
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < PERIOD_K; k++)
                if (k < K) acc[(size_t)k * n_members + m] = k == 2 ? PERIOD_WTD_NONE : 0;
        }
        if (B > 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) period_bin_add(period_bins, bin[q], lane);
        }
    }
#pragma unroll
    for (int k = 0; k < PERIOD_K; k++) {
        if (k < K) {
#pragma unroll
            for (int w = 0; w < HC_PROF_WORDS; w++) {
                long long v = words[k][w];
                for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) part[wave][k][w] = v;
            }
        }
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) counted += __shfl_xor(counted, o);
    if (lane == 0) cnt_part[wave] = counted;
    if (ovf) atomicAdd(&ovf_sum, ovf);
    if (outside) atomicAdd(&outside_sum, outside);
    __syncthreads();
    const size_t slot = (size_t)point * n_period + period;
    if ((int)threadIdx.x < K * HC_PROF_WORDS) {
        const int k = threadIdx.x / HC_PROF_WORDS, w = threadIdx.x % HC_PROF_WORDS;
        long long sum = 0;
#pragma unroll
        for (int u = 0; u < PERIOD_THREADS / WAVE; u++) sum += part[u][k][w];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(pmom + (slot * K + k) * HC_PROF_WORDS + w), (unsigned long long)sum);
    }
    if (B > 0) {
        int *tf = hist_flux + slot * 2 * B, *tw = hist_wtd + slot * 2 * D;
        for (int b = threadIdx.x; b < n_bins; b += PERIOD_THREADS) {
            const unsigned c = period_bins[b];
            if (c) atomicAdd(b < 2 * B ? tf + b : tw + (b - 2 * B), (int)c);
        }
    }
    if (threadIdx.x == 0) {
        long long n = 0;
#pragma unroll
        for (int u = 0; u < PERIOD_THREADS / WAVE; u++) n += cnt_part[u];
        if (n) atomicAdd(reinterpret_cast<unsigned long long *>(pcnt + slot), (unsigned long long)n);
        if (ovf_sum) atomicAdd(ovf_word, (unsigned long long)ovf_sum);
        if (B > 0 && outside_sum) atomicAdd(outside_word, (unsigned long long)outside_sum);
    }
}

// the particle filter's ancestry applied to the accumulators, next to filter_gather_kernel: slot m takes the K values of
// its ancestor (into the second buffer; the host swaps it in), each plane read through anc and written coalesced
__global__ void period_gather_kernel(const long long *anc, const long long *acc, long long *acc_out, long long n_members, int K)
{
    const size_t total = (size_t)n_members * K;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const long long m = (long long)(e % n_members), a = anc[m];
        acc_out[e] = acc[e - m + (a >= 0 && a < n_members ? a : m)];     // (every slot is filled: a guard)
    }
}

// The end of period `period` for the uptake: period_reduce_kernel's shape, launched before it (the members it counts are
// those period_reduce_kernel is about to count: wtd_shallowest != 65535 in the period accumulators `solved`).  A counted
// member enters umom [P][n_period][L + 1][5] with v_k = A_k >> 12 (floor; 2^-20 cm; clamped to HC_PROF_Q_MAX and counted)
// and, with B > 0, one entry per layer in bin min(B - 1, (v_l B) / v_0) of the block's LDS histogram uint32 [L][B] -- the
// layer's share of the member's total by integer division; a member with v_0 <= 0 adds one to `outside` instead.  The
// members of a point share a few bins a layer, so the lanes are grouped by bin first (period_bin_add).  Only nonzero
// words and bins go to the tables, with integer atomics.  Every member's accumulators are reset to 0.
__global__ __launch_bounds__(PERIOD_THREADS) void uptake_reduce_kernel(
    long long *uacc, const long long *solved, long long n_members, long long members_per_point, long long members_per_block,
    long long period, long long n_period, int L, int B, long long *umom, long long *ucnt, unsigned long long *ovf_word,
    int *hist, unsigned long long *outside_word)
{
    constexpr int K1 = HC_UPTAKE_MAX_LAYERS + 1;
    extern __shared__ unsigned uptake_bins[];        // [L][B]
    __shared__ long long part[PERIOD_THREADS / WAVE][K1][HC_PROF_WORDS];
    __shared__ long long cnt_part[PERIOD_THREADS / WAVE];
    __shared__ unsigned ovf_sum, outside_sum;
    const int n_bins = L * B;
    for (int b = threadIdx.x; b < n_bins; b += PERIOD_THREADS) uptake_bins[b] = 0;
    if (threadIdx.x == 0) ovf_sum = 0, outside_sum = 0;
    __syncthreads();
    const long long point = blockIdx.y;
    const long long end = (point + 1) * members_per_point;
    const long long m0 = point * members_per_point + (long long)blockIdx.x * members_per_block;
    const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const long long qmax = HC_PROF_Q_MAX;
    long long words[K1][HC_PROF_WORDS] = {};
    long long counted = 0;
    unsigned ovf = 0, outside = 0;
    // wave-uniform trip count: every lane of a wave runs the ballots of every round
    for (long long k0 = m0 + (threadIdx.x - lane); k0 < m1; k0 += PERIOD_THREADS) {
        const long long m = k0 + lane;
        const bool live = m < m1;
        long long v[K1];
#pragma unroll
        for (int k = 0; k < K1; k++) v[k] = (live && k <= L) ? uacc[(size_t)k * n_members + m] : 0;
        int bin[HC_UPTAKE_MAX_LAYERS];
#pragma unroll
        for (int l = 0; l < HC_UPTAKE_MAX_LAYERS; l++) bin[l] = -1;
        if (live && solved[m] != PERIOD_WTD_NONE) {
            counted++;
#pragma unroll
            for (int k = 0; k < K1; k++) {
                if (k <= L) {
                    v[k] >>= 12;                     // floor(A / 4096)
                    if (v[k] > qmax) v[k] = qmax, ovf++;
                    if (v[k] < -qmax) v[k] = -qmax, ovf++;
                    prof_add(words[k], v[k]);
                }
            }
            if (B > 0) {
                if (v[0] > 0) {
#pragma unroll
                    for (int l = 0; l < HC_UPTAKE_MAX_LAYERS; l++) {
                        if (l < L) {
                            const long long s = v[l + 1] < 0 ? 0 : (v[l + 1] * B) / v[0];
                            bin[l] = l * B + (int)(s < B - 1 ? s : B - 1);
                        }
                    }
                } else {
                    outside++;
                }
            }
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < K1; k++)
                if (k <= L) uacc[(size_t)k * n_members + m] = 0;
        }
        if (B > 0) {
#pragma unroll
            for (int l = 0; l < HC_UPTAKE_MAX_LAYERS; l++)
                if (l < L) period_bin_add(uptake_bins, bin[l], lane);
        }
    }
#pragma unroll
    for (int k = 0; k < K1; k++) {
        if (k <= L) {
#pragma unroll
            for (int w = 0; w < HC_PROF_WORDS; w++) {
                long long s = words[k][w];
                for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if (lane == 0) part[wave][k][w] = s;
            }
        }
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) counted += __shfl_xor(counted, o);
    if (lane == 0) cnt_part[wave] = counted;
    if (ovf) atomicAdd(&ovf_sum, ovf);
    if (outside) atomicAdd(&outside_sum, outside);
    __syncthreads();
    const size_t slot = (size_t)point * n_period + period;
    if ((int)threadIdx.x < (L + 1) * HC_PROF_WORDS) {
        const int k = threadIdx.x / HC_PROF_WORDS, w = threadIdx.x % HC_PROF_WORDS;
        long long sum = 0;
#pragma unroll
        for (int u = 0; u < PERIOD_THREADS / WAVE; u++) sum += part[u][k][w];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(umom + (slot * (L + 1) + k) * HC_PROF_WORDS + w), (unsigned long long)sum);
    }
    if (B > 0) {
        int *t = hist + slot * n_bins;
        for (int b = threadIdx.x; b < n_bins; b += PERIOD_THREADS) {
            const unsigned c = uptake_bins[b];
            if (c) atomicAdd(t + b, (int)c);
        }
    }
    if (threadIdx.x == 0) {
        long long n = 0;
#pragma unroll
        for (int u = 0; u < PERIOD_THREADS / WAVE; u++) n += cnt_part[u];
        if (n) atomicAdd(reinterpret_cast<unsigned long long *>(ucnt + slot), (unsigned long long)n);
        if (ovf_sum) atomicAdd(ovf_word, (unsigned long long)ovf_sum);
        if (B > 0 && outside_sum) atomicAdd(outside_word, (unsigned long long)outside_sum);
    }
}

struct WtdLevels {
    double q[HC_WTD_MAX_LEVELS];
};
constexpr int DIST_BINS = HC_MAX_DEPTH_NODES / WAVE;    // bins per lane at the deepest column

// 128-bit unsigned accumulator (hi, lo) += v
__device__ __forceinline__ void add_u128(unsigned long long &hi, unsigned long long &lo, unsigned long long vhi,
                                         unsigned long long vlo)
{
    lo += vlo;
    hi += vhi + (lo < vlo ? 1ull : 0ull);
}
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// dz S / n^2 for the exact S = (hi, lo): S and n^2 as double-double, one quotient, one rounding at the end
__device__ double crps_of(unsigned long long s_hi, unsigned long long s_lo, long long n, double dz)
{
    // S = a + b + c, each term exact in fp64 (S < 2^92: s_hi < 2^28)
    const double a = (double)s_hi * 0x1p64, b = (double)(s_lo >> 32) * 0x1p32, c = (double)(s_lo & 0xffffffffull);
    double s1, e1, s2, e2, x_hi, x_lo;
    two_sum(a, b, s1, e1);
    two_sum(s1, c, s2, e2);
    two_sum(s2, e1 + e2, x_hi, x_lo);
    const double nd = (double)n;                   // exact: n < 2^41
    const double d_hi = nd * nd, d_lo = fma(nd, nd, -d_hi);
    const double q1 = x_hi / d_hi;
    const double r = fma(-q1, d_hi, x_hi) + x_lo - q1 * d_lo;
    const double q2 = r / d_hi;
    const double p = q1 * dz, pe = fma(q1, dz, -p);
    return p + (pe + q2 * dz);
}

// The summary of hist [n_rows][D] (hc_wtd_distribution): one wavefront per row, grid-stride over the rows.  Lane l holds the
// contiguous bins [l per, (l + 1) per); a shuffle scan of the lane totals gives the cumulative counts; a quantile is the
// first bin whose cumulative count reaches k, one ballot per level; S is summed exactly in two 64-bit words per lane, then
// across the lanes.
__global__ __launch_bounds__(256) void wtd_dist_kernel(const int *hist, const int *obs_idx, long long n_rows, int D,
                                                       WtdLevels lv, int n_levels, double dz, long long *count,
                                                       int *quantile_idx, double *crps_cm)
{
    const int lane = threadIdx.x % WAVE;
    const long long waves = (long long)gridDim.x * (blockDim.x / WAVE);
    const int per = (D + WAVE - 1) / WAVE;
    for (long long row = (long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; row < n_rows; row += waves) {
        const int *hr = hist + (size_t)row * D;
        const int o = obs_idx[row];
        long long c[DIST_BINS];
        long long tot = 0;
#pragma unroll
        for (int t = 0; t < DIST_BINS; t++) {
            const int b = lane * per + t;
            if (t < per && b < D) tot += hr[b];
            c[t] = tot;
        }
        long long incl = tot;
        for (int d = 1; d < WAVE; d <<= 1) {
            const long long u = __shfl_up(incl, d);
            if (lane >= d) incl += u;
        }
        const long long excl = incl - tot;
        const long long n = __shfl(incl, WAVE - 1);
#pragma unroll
        for (int t = 0; t < DIST_BINS; t++) c[t] += excl;
        for (int l = 0; l < n_levels; l++) {
            int idx = -1;
            if (n > 0) {
                long long k = (long long)ceil((double)n * lv.q[l]);
                k = k < 1 ? 1 : k;
                int mine = -1;
#pragma unroll
                for (int t = DIST_BINS - 1; t >= 0; t--)
                    if (t < per && lane * per + t < D && c[t] >= k) mine = lane * per + t;
                const unsigned long long hit = __ballot(mine >= 0);
                idx = hit ? __shfl(mine, __ffsll((long long)hit) - 1) : -1;
            }
            if (lane == 0) quantile_idx[(size_t)row * n_levels + l] = idx;
        }
        unsigned long long s_hi = 0, s_lo = 0;
#pragma unroll
        for (int t = 0; t < DIST_BINS; t++) {
            const int b = lane * per + t;
            if (t < per && b < D - 1) {
                const long long d = c[t] - (b >= o ? n : 0);
                const unsigned long long m = (unsigned long long)(d < 0 ? -d : d);
                add_u128(s_hi, s_lo, __umul64hi(m, m), m * m);
            }
        }
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const unsigned long long ohi = __shfl_xor(s_hi, off), olo = __shfl_xor(s_lo, off);
            add_u128(s_hi, s_lo, ohi, olo);
        }
        if (lane == 0) {
            count[row] = n;
            crps_cm[row] = (n > 0 && o >= 0 && o < D) ? crps_of(s_hi, s_lo, n, dz) : __builtin_nan("");
        }
    }
}

// ---- particle filter on the well's water table (hc_set_filter, include/hydrocol.h)
// Everything the ancestry depends on is an integer: q_b, the prefix sums C_m, the draw r and the slot ranges.  The
// floating-point parts (l_b, W, the increment, the ESS quotient) run with contraction off, so that a NumPy restatement
// of the same expressions agrees to the last few ulps.
constexpr int FILT_THREADS = 256;
constexpr int FILT_PER_THREAD = 4;
constexpr long long FILT_TILE = FILT_THREADS * FILT_PER_THREAD;    // members per block of the prefix scan

// 128-bit unsigned integer -> (x_hi + x_lo) in double-double: four exact 32-bit limbs, summed with error terms
__device__ void u128_to_dd(unsigned long long hi, unsigned long long lo, double &x_hi, double &x_lo)
{
    const double v[4] = {(double)(hi >> 32) * 0x1p96, (double)(hi & 0xffffffffull) * 0x1p64, (double)(lo >> 32) * 0x1p32,
                         (double)(lo & 0xffffffffull)};
    double s = v[0], err = 0.0;
    for (int k = 1; k < 4; k++) {
        double t, e;
        two_sum(s, v[k], t, e);
        s = t;
        err += e;
    }
    two_sum(s, err, x_hi, x_lo);
}

// the Philox value of the filter's draw at (seed, point key, row).  The counter's first word is 0xFFFFFFFF: a noise
// draw's first word is a depth index / 2 (< HC_MAX_DEPTH_NODES / 2), so the two never share a counter under one key.
__device__ __forceinline__ unsigned long long filter_philox64(unsigned long long seed, unsigned long long point_key,
                                                              unsigned row)
{
    uint32_t r[4];
    philox4x32_10(0xFFFFFFFFu, row, (uint32_t)point_key, (uint32_t)(point_key >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    return ((unsigned long long)r[1] << 32) | r[0];
}

// ESS = Q^2 / sum q_m^2 (the sum in two 64-bit words): both exact, the quotient from a double-double correction (within
// 2 ulp)
__device__ __forceinline__ double filter_ess(unsigned long long Q, unsigned long long b_hi, unsigned long long b_lo)
{
#pragma clang fp contract(off)
    double a_hi, a_lo, d_hi, d_lo;
    u128_to_dd(__umul64hi(Q, Q), Q * Q, a_hi, a_lo);
    u128_to_dd(b_hi, b_lo, d_hi, d_lo);
    const double q1 = a_hi / d_hi;
    const double rr = fma(-q1, d_hi, a_hi) + a_lo - q1 * d_lo;
    return q1 + rr / d_hi;
}

// point p's draw: qr[p] = {Q, r} with r = floor(x Q / 2^64) < Q, x the Philox value under the point's key; the
// survivors' counter cleared
__device__ __forceinline__ void filter_draw(unsigned long long seed, const long long *point_base, long long member_offset,
                                            long long p, long long members_per_point, unsigned row, unsigned long long Q,
                                            unsigned long long *qr, unsigned long long *surv)
{
    const unsigned long long key = point_base ? (unsigned long long)point_base[p]
                                              : (unsigned long long)(member_offset + p * members_per_point);
    const unsigned long long x = filter_philox64(seed, key, row);
    qr[2 * p] = Q;
    qr[2 * p + 1] = __umul64hi(x, Q);
    surv[p] = 0;
}

// One block per point: bin counts n_b of the assimilation row's water-table indices (grouped by ballots as in
// wtd_hist_kernel), then one thread forms s, q_b, W, the exact sums of the ESS, the increment and the draw.
// qr[p] = {Q, r}; stats row = {count, ESS, increment, survivors (written by filter_fill_kernel's finish)}.
__global__ __launch_bounds__(FILT_THREADS) void filter_weights_kernel(
    const unsigned short *w, long long members_per_point, int D, int obs, double dz, double sigma, unsigned long long seed,
    const long long *point_base, long long member_offset, unsigned row, long long n_arow, long long slot, long long *q_out,
    unsigned long long *qr, double *stats, unsigned long long *surv)
{
#pragma clang fp contract(off)
    __shared__ unsigned bins[HC_MAX_DEPTH_NODES];
    __shared__ long long qsh[HC_MAX_DEPTH_NODES];
    for (int b = threadIdx.x; b < D; b += FILT_THREADS) bins[b] = 0;
    __syncthreads();
    const long long p = blockIdx.x;
    const long long m0 = p * members_per_point, m1 = m0 + members_per_point;
    const int lane = threadIdx.x % WAVE;
    for (long long k0 = m0 + (threadIdx.x - lane); k0 < m1; k0 += FILT_THREADS) {
        const long long k = k0 + lane;
        const int b = k < m1 ? (int)w[k] : -1;
        unsigned long long pending = __ballot(b >= 0 && b < D);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int v = __builtin_amdgcn_readlane(b, leader);
            const unsigned long long same = __ballot(b == v) & pending;
            if (lane == leader) atomicAdd(&bins[v], (unsigned)__popcll(same));
            pending &= ~same;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // l_b = -0.5 (dz (b - o) / sigma)^2; s = max over the occupied bins
        double s = -INFINITY;
        long long n = 0;
        for (int b = 0; b < D; b++)
            if (bins[b]) {
                const double t = dz * (double)(b - obs) / sigma;
                const double l = -0.5 * (t * t);
                s = l > s ? l : s;
                n += bins[b];
            }
        double W = 0.0;
        unsigned long long Q = 0, b_hi = 0, b_lo = 0;
        for (int b = 0; b < D; b++) {
            long long q = 0;
            if (bins[b]) {
                const double t = dz * (double)(b - obs) / sigma;
                const double e = exp(-0.5 * (t * t) - s);
                q = (long long)floor(0x1p31 * e);              // 2^31 at the nearest occupied bin, 0 below ~2^-31
                W += (double)bins[b] * e;
                const unsigned long long uq = (unsigned long long)q, nb = bins[b];
                Q += nb * uq;                                  // < 2^31 members x 2^31
                const unsigned long long sq = uq * uq;         // < 2^62
                add_u128(b_hi, b_lo, __umul64hi(sq, nb), sq * nb);
            }
            qsh[b] = q;
        }
        double *st = stats + ((size_t)p * n_arow + slot) * 4;
        st[0] = (double)n;
        if (n > 0 && Q > 0) {
            st[1] = filter_ess(Q, b_hi, b_lo);
            st[2] = s + log(W / (double)n) - log(sigma) - 0.5 * log(2.0 * M_PI);
        } else {
            st[1] = __builtin_nan("");
            st[2] = __builtin_nan("");
        }
        filter_draw(seed, point_base, member_offset, p, members_per_point, row, Q, qr, surv);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < D; b += FILT_THREADS) q_out[(size_t)p * D + b] = qsh[b];
}

// q_m of member k (handle-local) = q_{b_m} from the point's bin table q; w == NULL: the per-member weights of a sensor row
// (filter_member_weights_kernel), q being the handle's vector [n_members] then (filter_point_q)
__device__ __forceinline__ long long filter_q(const unsigned short *w, const long long *q, int D, long long k)
{
    if (!w) return q[k];
    const int b = (int)w[k];
    return b < D ? q[b] : 0;
}

// the table filter_q reads for point p: its row of the bin table [P][D], or the per-member vector as a whole
__device__ __forceinline__ const long long *filter_point_q(const unsigned short *w, const long long *q_all, int D, long long p)
{
    return w ? q_all + (size_t)p * D : q_all;
}

// inclusive wave64 scan of one value per lane (shuffles), then the block's exclusive offsets through LDS
__device__ __forceinline__ long long block_exclusive_scan(long long v, long long &total)
{
    __shared__ long long wsum[FILT_THREADS / WAVE];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    long long incl = v;
    for (int d = 1; d < WAVE; d <<= 1) {
        const long long u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    long long before = 0;
    total = 0;
    for (int u = 0; u < FILT_THREADS / WAVE; u++) {
        if (u < wave) before += wsum[u];
        total += wsum[u];
    }
    __syncthreads();              // wsum may be reused by the next call
    return before + incl - v;
}

// the sum of q_m over each tile of FILT_TILE members of a point: tiles[p][t]
__global__ __launch_bounds__(FILT_THREADS) void filter_tile_sum_kernel(const unsigned short *w, const long long *q_all,
                                                                       long long members_per_point, int D, long long n_tiles,
                                                                       long long *tiles)
{
    const long long p = blockIdx.y, t = blockIdx.x;
    const long long *q = filter_point_q(w, q_all, D, p);
    const long long first = p * members_per_point, m0 = t * FILT_TILE;
    long long v = 0;
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = m0 + (long long)threadIdx.x * FILT_PER_THREAD + j;
        if (m < members_per_point) v += filter_q(w, q, D, first + m);
    }
    long long total;
    (void)block_exclusive_scan(v, total);
    if (threadIdx.x == 0) tiles[(size_t)p * n_tiles + t] = total;
}

// the block-offset pass: tiles[p][*] -> their exclusive prefix sums, one block per point in rounds of FILT_THREADS tiles
__global__ __launch_bounds__(FILT_THREADS) void filter_tile_scan_kernel(long long n_tiles, long long *tiles)
{
    long long *t = tiles + (size_t)blockIdx.x * n_tiles;
    long long carry = 0;
    for (long long k0 = 0; k0 < n_tiles; k0 += FILT_THREADS) {
        const long long k = k0 + threadIdx.x;
        const long long v = k < n_tiles ? t[k] : 0;
        long long total;
        const long long ex = block_exclusive_scan(v, total);
        if (k < n_tiles) t[k] = carry + ex;
        carry += total;
    }
}

// Member m of point p (C_m = its exclusive prefix sum of q in member order) fills the slots
// k in [ceil((C_m N_p - r) / Q), ceil(((C_m + q_m) N_p - r) / Q)) with its handle-local index; survivors are counted.
__device__ __forceinline__ long long filter_slot(unsigned long long c, unsigned long long Np, unsigned long long r,
                                                 unsigned long long Q)
{
    const unsigned __int128 num = (unsigned __int128)c * Np;
    if (num <= r) return 0;
    return (long long)((num - r + (Q - 1)) / Q);
}

__global__ __launch_bounds__(FILT_THREADS) void filter_fill_kernel(const unsigned short *w, const long long *q_all,
                                                                   long long members_per_point, int D, long long n_tiles,
                                                                   const long long *tiles, const unsigned long long *qr,
                                                                   long long *anc, unsigned long long *surv)
{
    const long long p = blockIdx.y, t = blockIdx.x;
    const long long *q = filter_point_q(w, q_all, D, p);
    const long long first = p * members_per_point, m0 = t * FILT_TILE + (long long)threadIdx.x * FILT_PER_THREAD;
    const unsigned long long Q = qr[2 * p], r = qr[2 * p + 1], Np = (unsigned long long)members_per_point;
    long long qm[FILT_PER_THREAD], v = 0;
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = m0 + j;
        qm[j] = m < members_per_point ? filter_q(w, q, D, first + m) : 0;
        v += qm[j];
    }
    long long total;
    unsigned long long c = (unsigned long long)(tiles[(size_t)p * n_tiles + t] + block_exclusive_scan(v, total));
    unsigned alive = 0;
    const int lane = threadIdx.x % WAVE;
    // every lane runs every round (ballots below): members past the point's end have an empty range
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = m0 + j;
        long long k0 = 0, k1 = 0;
        if (m < members_per_point) {
            if (Q == 0) {                   // no member counted: the ancestry stays the identity
                k0 = m, k1 = m + 1;
            } else {
                k0 = filter_slot(c, Np, r, Q);
                k1 = filter_slot(c + (unsigned long long)qm[j], Np, r, Q);
            }
            k1 = k1 < members_per_point ? k1 : members_per_point;
        }
        // a short range is written by its own lane; a long one (weight concentrated on a few members: up to N_p slots)
        // by the whole wave, one such range after the other, 64 consecutive slots per store
        const bool wide = k1 - k0 > WAVE;
        if (!wide)
            for (long long k = k0; k < k1; k++) anc[first + k] = first + m;
        for (unsigned long long pend = __ballot(wide); pend; pend &= pend - 1) {
            const int src = __ffsll((long long)pend) - 1;
            const long long a = __shfl(k0, src), b = __shfl(k1, src), v = __shfl(first + m, src);
            for (long long k = a + lane; k < b; k += WAVE) anc[first + k] = v;
        }
        alive += k1 > k0 ? 1u : 0u;
        c += m < members_per_point ? (unsigned long long)qm[j] : 0ull;
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) alive += __shfl_xor(alive, o);
    if (threadIdx.x % WAVE == 0 && alive) atomicAdd(surv + p, (unsigned long long)alive);
}

__global__ void filter_survivors_kernel(const unsigned long long *surv, int n_points, long long n_arow, long long slot,
                                        double *stats)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_points) stats[((size_t)p * n_arow + slot) * 4 + 3] = (double)surv[p];
}

// slot k takes the state and the base noise vector of its ancestor (into the second buffers; the host swaps them in)
__global__ void filter_gather_kernel(const long long *anc, const double *psi, const double *base, double *psi_out,
                                     double *base_out, long long n_members, int D)
{
    const size_t total = (size_t)n_members * D;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const long long k = (long long)(e / D), a = anc[k];
        const size_t src = (size_t)(a >= 0 && a < n_members ? a : k) * D + e % D;     // (every slot is filled: a guard)
        psi_out[e] = psi[src];
        if (base) base_out[e] = base[src];
    }
}

// ---- one point's members on several handles (hc_set_filter_shard, include/hydrocol.h): integers and 8-byte copies only.
// Every handle computes the point's whole ancestry anc[n_global] from the gathered water-table indices.  Systematic
// resampling is monotone -- anc[k] is non-decreasing in k -- so equal ancestors are neighbours, the slots of a shard
// that take their column from another shard's members form one run, and both ends of a transfer derive the same list
// of members (the distinct ancestors of the run, ascending) from the same table.

// the handle's water-table indices of the row as 8-byte words at their place in the gathered vector
__global__ void filter_shard_index_kernel(const unsigned short *w, long long n, long long *idx)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) idx[k] = (long long)w[k];
}

// ... and the gathered vector as the ancestry kernels read it
__global__ void filter_shard_narrow_kernel(const long long *idx, long long n_global, unsigned short *w)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_global) w[k] = (unsigned short)idx[k];
}

// Slot k opens a run when k = 0 or anc[k] != anc[k - 1].  rank == NULL: the runs opened in each tile of FILT_TILE slots
// -> tiles[t]; else, tiles[] being their exclusive prefix sums (filter_tile_scan_kernel), rank[k] = the runs opened in
// [0, k], less one: the index of anc[k] among the distinct ancestors.
__global__ __launch_bounds__(FILT_THREADS) void filter_shard_rank_kernel(const long long *anc, long long n_global,
                                                                         long long *tiles, long long *rank)
{
    const long long k0 = (long long)blockIdx.x * FILT_TILE + (long long)threadIdx.x * FILT_PER_THREAD;
    long long prev = k0 > 0 && k0 < n_global ? anc[k0 - 1] : -1, v = 0;
    bool opens[FILT_PER_THREAD];
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long k = k0 + j;
        opens[j] = false;
        if (k < n_global) {
            const long long a = anc[k];
            opens[j] = k == 0 || a != prev;
            prev = a;
        }
        v += opens[j] ? 1 : 0;
    }
    long long total;
    const long long before = block_exclusive_scan(v, total);
    if (!rank) {
        if (threadIdx.x == 0) tiles[blockIdx.x] = total;
        return;
    }
    long long c = tiles[blockIdx.x] + before;
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long k = k0 + j;
        c += opens[j] ? 1 : 0;
        if (k < n_global) rank[k] = c - 1;
    }
}

// the first index in [lo, hi) of the non-decreasing a[] whose entry is >= v (hi: none)
__device__ __forceinline__ long long filter_lower_bound(const long long *a, long long lo, long long hi, long long v)
{
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the shard that holds member (or slot) v: bounds[s] <= v < bounds[s + 1]
__device__ __forceinline__ int filter_shard_of(const long long *bounds, int S, long long v)
{
    return (int)filter_lower_bound(bounds + 1, 0, S - 1, v + 1);
}

// the distinct ancestors that the slots [k0, k1) have in [m0, m1), and the first such slot
__device__ __forceinline__ long long filter_run(const long long *anc, const long long *rank, long long k0, long long k1,
                                                long long m0, long long m1, long long &lo)
{
    lo = filter_lower_bound(anc, k0, k1, m0);
    const long long hi = filter_lower_bound(anc, lo, k1, m1);
    return hi > lo ? rank[hi - 1] - rank[lo] + 1 : 0;
}

// The routing table [6][S] of shard `me`, one thread per other shard s: the members it receives from s (rows 0 and 2)
// and sends to s (rows 1 and 3), and the first slot of either run (rows 4 and 5).  filter_tile_scan_kernel then turns
// rows 2 and 3 into the offsets of the blocks in the receive and the send region, in members.
__global__ void filter_route_kernel(const long long *anc, const long long *rank, const long long *bounds, int S, int me,
                                    long long *table)
{
    const long long first = bounds[me], last = bounds[me + 1];
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < S; s += gridDim.x * blockDim.x) {
        long long lo_r = first, lo_s = bounds[s], n_r = 0, n_s = 0;
        if (s != me) {
            n_r = filter_run(anc, rank, first, last, bounds[s], bounds[s + 1], lo_r);
            n_s = filter_run(anc, rank, bounds[s], bounds[s + 1], first, last, lo_s);
        }
        table[s] = table[2 * S + s] = n_r;
        table[S + s] = table[3 * S + s] = n_s;
        table[4 * S + s] = lo_r;
        table[5 * S + s] = lo_s;
    }
}

// Every slot of the point, from the routing table.  One of the handle's own: its source, src[k - first] = the local
// member, or -1 - j for entry j of the receive region.  Another shard's slot that opens a run of one of the handle's
// members: that member into the list of columns to pack, at the run's place in the destination's block.  (A table that
// is not an ancestry -- a gather that did not deliver -- writes nothing out of bounds: such a slot keeps its own column.)
__global__ void filter_route_fill_kernel(const long long *anc, const long long *rank, const long long *bounds, int S, int me,
                                         const long long *table, long long n_global, long long *list, long long list_cap,
                                         long long *src)
{
    const long long first = bounds[me], last = bounds[me + 1], n = last - first;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_global; k += (long long)gridDim.x * blockDim.x) {
        const long long a = anc[k];
        const bool local = a >= first && a < last;
        if (k >= first && k < last) {
            long long from = k - first;
            if (local) {
                from = a - first;
            } else if (a >= 0 && a < n_global) {
                const int s = filter_shard_of(bounds, S, a);
                const long long lo = table[4 * S + s];
                const long long j = lo <= k ? table[2 * S + s] + rank[k] - rank[lo] : -1;
                if (j >= 0 && j < n) from = -1 - j;
            }
            src[k - first] = from;
        } else if (local) {
            const int d = filter_shard_of(bounds, S, k);
            if (k == bounds[d] || anc[k - 1] != a) {
                const long long lo = table[5 * S + d];
                const long long j = lo <= k ? table[3 * S + d] + rank[k] - rank[lo] : -1;
                if (j >= 0 && j < list_cap) list[j] = a - first;
            }
        }
    }
}

// the listed members' columns into the send region, psi[D] then base[D] per member, as 8-byte words
__global__ void filter_pack_kernel(const long long *list, const long long *table, int S, long long list_cap, long long n,
                                   const long long *psi, const long long *base, long long *send, int D)
{
    long long n_list = table[3 * S + S - 1] + table[S + S - 1];
    n_list = n_list < list_cap ? n_list : list_cap;
    const size_t total = (size_t)(n_list > 0 ? n_list : 0) * 2 * D;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const long long m = list[e / (2 * (size_t)D)];
        const int c = (int)(e % (2 * (size_t)D));
        if (m < 0 || m >= n) continue;
        send[e] = c < D ? psi[(size_t)m * D + c] : base[(size_t)m * D + (c - D)];
    }
}

// slot k takes psi and base from the handle's own member src[k], or from entry -1 - src[k] of the receive region
// (into the second buffers, as filter_gather_kernel does)
__global__ void filter_shard_gather_kernel(const long long *src, const long long *psi, const long long *base,
                                           const long long *recv, long long *psi_out, long long *base_out, long long n, int D)
{
    const size_t total = (size_t)n * D;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const long long s = src[e / D];
        const size_t i = e % D;
        if (s >= 0) {
            psi_out[e] = psi[(size_t)s * D + i];
            base_out[e] = base[(size_t)s * D + i];
        } else {
            const size_t at = (size_t)(-1 - s) * 2 * D + i;
            psi_out[e] = recv[at];
            base_out[e] = recv[at + D];
        }
    }
}

// a filtered Philox run hands the step kernel caller-style noise made from the kernel's own normals: n_vec vectors
// [n_vec][N][D]; rows == NULL: the base vectors (draw 0) times the member's scale, else the refresh rows rows[v] with
// their draw indices.  A member's stream is keyed by its slot (member_offset + m, or the point's base + j).
__global__ void filter_philox_fill_kernel(double *out, long long n_vec, const long long *rows, const int *draw_idx,
                                          unsigned long long seed, long long member_offset, const long long *point_base,
                                          long long members_per_point, long long n_members, int D, const double *nscale)
{
    const size_t per = (size_t)n_members * D, total = per * (size_t)n_vec;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const long long v = (long long)(e / per), m = (long long)((e % per) / D);
        const int i = (int)(e % D);
        const unsigned draw = rows ? (unsigned)draw_idx[rows[v]] : 0u;
        const long long gid = point_base ? point_base[m / members_per_point] + m % members_per_point : member_offset + m;
        const double z = philox_normal(seed, (unsigned long long)gid, draw, (unsigned)i);
        out[e] = nscale ? z * nscale[m] : z;
    }
}

// ---- correlated noise fields (hc_set_noise_correlation; include/hydrocol.h)
// filter_philox_fill_kernel's job with a vertical correlation: the same vectors [n_vec][N][D] from the same streams, each
// run through the point's recursion  z_i = xi_i where a_i == 0, else (a_i z_{i-1}) + (b_i xi_i)  down the column, in one
// pass.  A work item is one vector's tile of NF_TILE members of one point (a tile never spans two points: a, b are the
// point's), taken NF_CHUNK nodes at a time through LDS:
//   all waves draw the chunk's normals, one Philox block per node pair as philox_normal pairs them (cosine to the even
//   node, sine to the odd one: xi is philox_normal's to the bit), into tile[member][node];
//   the first wave walks one member per lane down the chunk in node order, z_{i-1} carried in a register from chunk to
//   chunk (lane stride NF_PITCH = 65 doubles: the 32 lanes of a ds_read_b64 group fall on 32 distinct bank pairs);
//   all waves store the tile, one member's 64 contiguous doubles per wave instruction.
// One block per work item (a grid-stride loop over the items cost 20 SGPRs and nine of them spilled).
// The third barrier of a chunk keeps the next chunk's draws out of a tile that is still being stored.
constexpr int NF_TILE = 64, NF_CHUNK = 64, NF_PITCH = NF_CHUNK + 1, NF_THREADS = 256;

// philox_normal's two values of one counter block: nodes 2 k and 2 k + 1
__device__ __forceinline__ void philox_normal_pair(uint64_t seed, uint64_t member, uint32_t draw, uint32_t k, double &even,
                                                   double &odd)
{
    uint32_t r[4];
    philox4x32_10(k, draw, (uint32_t)member, (uint32_t)(member >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    uint64_t a = ((uint64_t)r[1] << 32) | r[0], b = ((uint64_t)r[3] << 32) | r[2];
    double u1 = ((double)(a >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    double u2 = ((double)(b >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    even = rad * c;
    odd = rad * s;
}

__global__ __launch_bounds__(NF_THREADS) void noise_field_fill_kernel(
    double *out, long long n_vec, const long long *rows, const int *draw_idx, unsigned long long seed, long long member_offset,
    const long long *point_base, long long members_per_point, long long n_members, int D, const double *nscale,
    const double *a, const double *b)
{
#pragma clang fp contract(off)
    __shared__ double tile[NF_TILE * NF_PITCH];
    __shared__ double ab[2][NF_CHUNK];
    const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    const long long n_points = n_members / members_per_point;
    const long long tiles = (members_per_point + NF_TILE - 1) / NF_TILE, per_vec = n_points * tiles;
    const long long w = blockIdx.x;             // (the host launches one block per work item)
    if (w >= n_vec * per_vec) return;
    const long long v = w / per_vec, point = (w % per_vec) / tiles, j0 = (w % tiles) * NF_TILE;
    const int n_mem = (int)(members_per_point - j0 < NF_TILE ? members_per_point - j0 : NF_TILE);
    const long long m0 = point * members_per_point + j0;                    // the tile's first slot
    const unsigned long long gid0 = (unsigned long long)((point_base ? point_base[point] : member_offset) + j0);
    const unsigned draw = rows ? (unsigned)draw_idx[rows[v]] : 0u;
    const double *ap = a + (size_t)point * D, *bp = b + (size_t)point * D;
    double *dst = out + ((size_t)v * n_members + m0) * D;
    double zprev = 0.0;                                                     // (a_0 == 0: never read at node 0)
    for (int c0 = 0; c0 < D; c0 += NF_CHUNK) {
        const int len = D - c0 < NF_CHUNK ? D - c0 : NF_CHUNK;
        if (wave == 1 && lane < len) ab[0][lane] = ap[c0 + lane];
        if (wave == 2 && lane < len) ab[1][lane] = bp[c0 + lane];
#pragma unroll 1
        for (int q = t; q < NF_TILE * (NF_CHUNK / 2); q += NF_THREADS) {
            const int ml = q / (NF_CHUNK / 2), j = 2 * (q % (NF_CHUNK / 2));
            if (ml < n_mem && j < len) {
                double even, odd;
                philox_normal_pair(seed, gid0 + ml, draw, (unsigned)(c0 + j) >> 1, even, odd);
                tile[ml * NF_PITCH + j] = even;
                if (j + 1 < len) tile[ml * NF_PITCH + j + 1] = odd;
            }
        }
        __syncthreads();
        if (t < n_mem) {
            double *row = tile + t * NF_PITCH;
            for (int j = 0; j < len; j++) {
                const double aj = ab[0][j], xi = row[j];
                const double z = aj == 0.0 ? xi : (aj * zprev) + (ab[1][j] * xi);
                row[j] = z;
                zprev = z;
            }
        }
        __syncthreads();
        if (lane < len)
            for (int ml = wave; ml < n_mem; ml += NF_THREADS / WAVE) {
                const double z = tile[ml * NF_PITCH + lane];
                dst[(size_t)ml * D + c0 + lane] = nscale ? z * nscale[m0 + ml] : z;
            }
        __syncthreads();
    }
}

// a diagnostics table of `width` entries per slot, created as NaN but for each slot's first entry, the count, created as 0
// (the particle filter's and the EnKF's); width 0: all NaN (the sensors')
__global__ void stats_init_kernel(double *stats, size_t n, int width)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) stats[k] = width > 0 && k % width == 0 ? 0.0 : __builtin_nan("");
}

// ---- ensemble Kalman filter (hc_set_enkf, hc_set_enkf_soil_moisture; include/hydrocol.h)
// An analysis row runs a batch analysis of m' = 1 + m_s observations per member: the well's y, then the theta of the
// soil-moisture sensors with a value on the row (m_s = 0: the well alone).  Depths are measured from the top node,
// z_i = i dz: the C-ABI knows no z[0], and every quantity but the two means of the diagnostics is a difference of depths
// (the host adds z[0] to those).  Every sum over a point's members runs in an order fixed by N_p alone -- tiles of
// ENKF_TILE members summed in member order, then the tile partials by ENKF_THREADS threads in tile-strided order and a
// fixed tree, for every column at once -- and no floating-point atomics, so the analysis is the same at any launch
// length, point order or member split.  The small m' x m' system is factorised by one thread per point.  Contraction is
// off throughout (but inside the cell model, which keeps the code generation of model_nodes_kernel).
constexpr int ENKF_TILE = 256;                         // members per partial of the column sums
constexpr int ENKF_THREADS = 1024;                     // the sums of the tile partials
constexpr int ENKF_SLOTS = HC_MAX_DEPTH_NODES / WAVE;  // depth nodes per lane of the update (one wave per member)
constexpr int ENKF_WIDTH = 8;                          // diagnostics per point and slot
constexpr int ENKF_FORCING_WIDTH = 9;                  // forcing-state diagnostics per point and slot (hc_set_enkf_forcing)
constexpr int ENKF_SENSORS = 8;                        // sensors in a record
constexpr int ENKF_OBS = ENKF_SENSORS + 1;             // observations per member: the well, then the sensors present
constexpr int ENKF_SENSOR_WIDTH = 6;                   // sensor diagnostics per point, slot and sensor

constexpr int ENKF_WINDOW_WIDTH = 4;                   // window diagnostics per point, slot and offset

// the observations of one analysis row beyond the well's (a kernel argument): the present sensors in record order, then
// the present lagged rows of the window by ascending offset (hc_set_enkf_window).  A row without a sensor value (ms = 0)
// leaves everything of the sensors -- their draws, their table -- untouched, and so does one without a lagged row
// (m = ms) for the window.  A lagged column k >= ms is a well-type observation: obs[k] = z[wtd_obs[r_j]] is also the
// centre of its taper, sigma[k] the well's sigma_cm, wrow[k] = r_j the row word of its draw.
struct EnkfRow {
    int m;                     // columns beyond the well's, m_s + m_w (m' = m + 1)
    int n;                     // sensors drawn for and recorded: the record's, 0 when ms = 0
    int sensor[ENKF_SENSORS];  // record index of present sensor k; k >= ms: the offset's index
    int node[ENKF_SENSORS];
    double obs[ENKF_SENSORS];
    double sigma[ENKF_SENSORS];
    int ms;                    // present sensors m_s
    int nw;                    // offsets recorded: the window's, 0 when m = ms
    unsigned wrow[ENKF_SENSORS];
};

// One standard normal of Philox4x32-10 under the EnKF seed at counter (word0, row, gid_lo, gid_hi), with the Box-Muller
// step of philox_normal (its cosine branch): the well's eps_k at word0 = 0xFFFFFFFE, sensor i's at 0xFFFFFFF0 + i.  A noise
// counter's first word is a depth index / 2 and the particle filter's draw has 0xFFFFFFFF: they never meet.  (The
// perturbed forcing's two streams have 0xFFFFFFE0 and 0xFFFFFFE1: HC_FORCING_WORD_PRECIP / _DEMAND.)
__device__ __forceinline__ double enkf_normal_at(uint32_t word0, unsigned long long seed, unsigned long long gid,
                                                 unsigned row)
{
#pragma clang fp contract(off)
    uint32_t r[4];
    philox4x32_10(word0, row, (uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const uint64_t a = ((uint64_t)r[1] << 32) | r[0], b = ((uint64_t)r[3] << 32) | r[2];
    const double u1 = ((double)(a >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(b >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    return sqrt(-2.0 * log(u1)) * c;
}

// the continuous water table of a column whose find_wtd index is b: where psi crosses psi_sat between nodes b - 1 and b,
// the linear interpolation of the crossing, in (z[b-1], z[b]]; else z[b]
__device__ __forceinline__ double enkf_y_of(int b, double lo, double hi, double psat, double dz)
{
#pragma clang fp contract(off)
    if (b >= 1 && lo < psat && psat <= hi) return (double)(b - 1) * dz + dz * (psat - lo) / (hi - lo);
    return (double)b * dz;
}

// Gaspari & Cohn (1999) eq. 4.10, the fifth-order taper with support 2 (r = distance / L)
__device__ __forceinline__ double gaspari_cohn(double r)
{
#pragma clang fp contract(off)
    if (r <= 1.0) return (((-0.25 * r + 0.5) * r + 0.625) * r - 5.0 / 3.0) * r * r + 1.0;
    if (r <= 2.0) return ((((r / 12.0 - 0.5) * r + 0.625) * r + 5.0 / 3.0) * r - 5.0) * r + 4.0 - 2.0 / (3.0 * r);
    return 0.0;
}

// Y[m][0] = y_m of every member (rows of `width` entries) from the index the step kernel wrote (wtd_u16's row) and the two
// nodes around it
__global__ void enkf_obs_kernel(const unsigned short *w, const double *psi, const ColumnDev *P, long long n_members,
                                long long mpp, int D, double dz, double *Y, int width)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const int b = (int)w[m] < D ? (int)w[m] : D - 1;
    const double *col = psi + (size_t)m * D;
    Y[(size_t)m * width] = enkf_y_of(b, b >= 1 ? col[b - 1] : 0.0, col[b], P[m / mpp].psi_sat, dz);
}

// the sum over the block's threads in a fixed tree (every thread gets it)
__device__ double enkf_block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = ENKF_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// theta of one cell as model_nodes_kernel computes it (theta has no noise term)
__device__ __forceinline__ double enkf_theta(const ColumnDev &P, const double *nt, int D, int j, double psi, int special)
{
    const double por = nt[j], meank = nt[D + j], noisec = nt[2 * D + j];
    const double mk = meank == 0.0 ? 1.0e-7 : meank;
    double th, K, C, kb, pf;
    if (special)
        model_cell<true>(P, psi, por, 1.0 / (por - P.theta_res), log(mk), 1.0 / (mk * mk), noisec, 0.0, th, K, C, kb, pf);
    else
        model_cell<false>(P, psi, por, 1.0 / (por - P.theta_res), log(mk), 1.0 / (mk * mk), noisec, 0.0, th, K, C, kb, pf);
    return th;
}

// Y[m][1 + k] = theta of member m at the node of present sensor k, rows of `width` entries: the forecast's Y (width m')
// and the posterior's (y, theta..., rejected)
__global__ void enkf_theta_kernel(const double *psi, const ColumnDev *P, const double *node_tabs, int special,
                                  long long n_members, long long mpp, int D, const EnkfRow s, double *Y, int width)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const long long p = m / mpp;
    const double *nt = node_tabs + (size_t)p * 3 * D;
    for (int k = 0; k < s.ms; k++)
        Y[(size_t)m * width + 1 + k] = enkf_theta(P[p], nt, D, s.node[k], psi[(size_t)m * D + s.node[k]], special);
}

// Y[m][1 + k] = the y that member m had on lagged row k (k >= ms), as enkf_obs_kernel left it in the window's buffer
// [offsets][N] when that row was solved
__global__ void enkf_window_gather_kernel(const double *win_y, long long n_members, const EnkfRow s, double *Y, int width)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    for (int k = s.ms; k < s.m; k++) Y[(size_t)m * width + 1 + k] = win_y[(size_t)s.sensor[k] * n_members + m];
}

// Column sums of X = (psi_0 .. psi_{Dc-1}, Y_0 .. Y_{W-1}) (Dc = 0: Y alone), C = Dc + W columns.  Block (t, p) takes
// tile t of point p's mpp members on this handle; they are tiles tile0, tile0 + 1, ... of a point with np members and
// n_tiles tiles (the whole point: np = mpp, tile0 = 0; hc_set_enkf_shard: a part of it, and p = 0), to = tile0 + t:
//   sums == NULL: partial[p][to][j] = sum over the tile in member order of X_j;
//   otherwise:    partial[p][to][j][i] = sum of (X_j - xbar_j)(Y_i - ybar_i), the means = sums[p][.] / np; and with
//                 SQUARE (the relaxation to prior spread): square[p][to][j] = sum of (psi_j - psibar_j)^2, j < Dc.
// Thread j owns column j: every member's psi row is one coalesced read of the block, and the tile offset is uniform
// over the block, so its stores are coalesced wherever the tile lands.
template <bool SQUARE>
__global__ __launch_bounds__(HC_MAX_DEPTH_NODES + WAVE) void enkf_partial_kernel(const double *psi, const double *Y, int W,
                                                                                 const double *sums, long long mpp, int Dc,
                                                                                 long long n_tiles, double *partial,
                                                                                 double *square, long long np,
                                                                                 long long tile0)
{
#pragma clang fp contract(off)
    const long long p = blockIdx.y, t = blockIdx.x, to = tile0 + t;
    const int j = threadIdx.x, C = Dc + W;
    if (j >= C) return;
    const long long m0 = p * mpp + t * ENKF_TILE;
    const long long m1 = p * mpp + ((t + 1) * ENKF_TILE < mpp ? (t + 1) * ENKF_TILE : mpp);
    const double *x = j < Dc ? psi + j : Y + (j - Dc);
    const long long xs = j < Dc ? Dc : W;
    if (!sums) {
        double s = 0.0;
#pragma unroll 8
        for (long long m = m0; m < m1; m++) s += x[(size_t)m * xs];
        partial[((size_t)p * n_tiles + to) * C + j] = s;
        return;
    }
    const double *S = sums + (size_t)p * C;
    const double xb = S[j] / (double)np;
    double yb[ENKF_OBS + 1], acc[ENKF_OBS + 1];
#pragma unroll
    for (int i = 0; i < ENKF_OBS + 1; i++) {
        yb[i] = i < W ? S[Dc + i] / (double)np : 0.0;
        acc[i] = 0.0;
    }
    double sq = 0.0;
    for (long long m = m0; m < m1; m++) {
        const double a = x[(size_t)m * xs] - xb;
        const double *ym = Y + (size_t)m * W;
#pragma unroll
        for (int i = 0; i < ENKF_OBS + 1; i++)
            if (i < W) acc[i] += a * (ym[i] - yb[i]);
        if (SQUARE) sq += a * a;
    }
    if (SQUARE && j < Dc) square[((size_t)p * n_tiles + to) * Dc + j] = sq;
    double *out = partial + (((size_t)p * n_tiles + to) * C + j) * W;
#pragma unroll
    for (int i = 0; i < ENKF_OBS + 1; i++)
        if (i < W) out[i] = acc[i];
}

// sums[p][c] = the tile partials of column c summed (thread t: tiles t, t + ENKF_THREADS, ... in order, then a fixed tree)
__global__ __launch_bounds__(ENKF_THREADS) void enkf_finish_kernel(const double *partial, long long n_tiles, int n_cols,
                                                                   double *sums)
{
#pragma clang fp contract(off)
    __shared__ double sh[ENKF_THREADS];
    const long long p = blockIdx.y;
    const int c = blockIdx.x;
    double part = 0.0;
    for (long long t = threadIdx.x; t < n_tiles; t += ENKF_THREADS) part += partial[((size_t)p * n_tiles + t) * n_cols + c];
    const double s = enkf_block_sum(part, sh);
    if (threadIdx.x == 0) sums[(size_t)p * n_cols + c] = s;
}

// L L^T = A (n x n, row-major, lower triangle read), in a fixed order; false when a pivot is not finite and > 0
__device__ bool enkf_cholesky(const double *A, int n, double *L)
{
#pragma clang fp contract(off)
    for (int j = 0; j < n; j++) {
        double d = A[j * ENKF_OBS + j];
        for (int k = 0; k < j; k++) d -= L[j * ENKF_OBS + k] * L[j * ENKF_OBS + k];
        if (!(d > 0.0) || !isfinite(d)) return false;
        const double ljj = sqrt(d);
        L[j * ENKF_OBS + j] = ljj;
        for (int i = j + 1; i < n; i++) {
            double v = A[i * ENKF_OBS + j];
            for (int k = 0; k < j; k++) v -= L[i * ENKF_OBS + k] * L[j * ENKF_OBS + k];
            L[i * ENKF_OBS + j] = v / ljj;
        }
    }
    return true;
}

// One block per point, thread d = node d.  Thread 0: ybar, C_YY, the tapered S = rho o C_YY + R and its Cholesky factor;
// the untapered C_YY + R for the joint log-density; the prior diagnostics (EnKF entries 0-4, the sensors' first four).
// Then thread d: K_d = (rho_d o c_d) S^-1 by a forward and a backward substitution, into gain[p][i][d].  The square-root
// analysis (rgain != NULL) also takes the mean's increment dbar[p][d] = sum_i K_di (o_i - Ybar_i), i in order, and the
// reduced gain Kr_d = (rho_d o c_d) L^-T (L + R^1/2)^-1 into rgain[p][i][d]: the forward substitution once more, then a
// backward substitution with the lower-triangular L + R^1/2 (the same LDS working set).
// stats == NULL (the noise field's gain, hc_set_enkf_noise_field: s1 and s2 are the sums over (z, Y), whose Y block is
// the state's to the bit, and so is the factor): no table is written.  taper_x = 0 (the forcing state's gain,
// hc_set_enkf_forcing: its D = 2 rows have no depth): rho_d = 1, while S keeps its taper.
__global__ __launch_bounds__(HC_MAX_DEPTH_NODES) void enkf_gain_kernel(const double *s1, const double *s2, long long mpp,
                                                                       int D, const EnkfRow s, double sigma, double loc,
                                                                       double z_obs, double dz, double *gain,
                                                                       double *stats, double *sm_stats, long long n_arow,
                                                                       long long slot, double *rgain, double *dbar,
                                                                       double *win_stats, int taper_x)
{
#pragma clang fp contract(off)
    // the working sets live in LDS (dynamically indexed: in registers they would go to scratch)
    __shared__ double Ls[ENKF_OBS * ENKF_OBS], Lu[ENKF_OBS * ENKF_OBS], A[ENKF_OBS * ENKF_OBS], cyy[ENKF_OBS * ENKF_OBS];
    __shared__ double zeta[ENKF_OBS], yb[ENKF_OBS], r2[ENKF_OBS], dl[ENKF_OBS], w[ENKF_OBS];
    __shared__ double U[HC_MAX_DEPTH_NODES][ENKF_OBS];   // thread d's substitutions
    __shared__ int ok;
    const long long p = blockIdx.x;
    const int W = s.m + 1, C = D + W;
    const double *S1 = s1 + (size_t)p * C, *S2 = s2 + (size_t)p * C * W;
    const double n1 = mpp > 1 ? (double)(mpp - 1) : 0.0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < W; i++) {
            yb[i] = S1[D + i] / (double)mpp;
            r2[i] = i == 0 ? sigma * sigma : s.sigma[i - 1] * s.sigma[i - 1];
            dl[i] = (i == 0 ? z_obs : s.obs[i - 1]) - yb[i];
            zeta[i] = i == 0 ? yb[0] : i <= s.ms ? (double)s.node[i - 1] * dz : s.obs[i - 1];
        }
        for (int i = 0; i < W; i++)
            for (int k = 0; k < W; k++) cyy[i * ENKF_OBS + k] = mpp > 1 ? S2[(size_t)(D + i) * W + k] / n1 : 0.0;
        for (int i = 0; i < W; i++)
            for (int k = 0; k < W; k++) {
                const double rho = loc > 0.0 ? gaspari_cohn(fabs(zeta[i] - zeta[k]) / loc) : 1.0;
                A[i * ENKF_OBS + k] = rho * cyy[i * ENKF_OBS + k] + (i == k ? r2[i] : 0.0);
            }
        ok = enkf_cholesky(A, W, Ls) ? 1 : 0;
        // log N(obs; ybar, C_YY + R) = -0.5 (m' log 2 pi + log det + |L^-1 (obs - ybar)|^2)
        for (int i = 0; stats && i < W; i++)
            for (int k = 0; k < W; k++) A[i * ENKF_OBS + k] = cyy[i * ENKF_OBS + k] + (i == k ? r2[i] : 0.0);
        double ll = __builtin_nan("");
        if (stats && enkf_cholesky(A, W, Lu)) {
            double logdet = 0.0, q = 0.0;
            for (int i = 0; i < W; i++) {
                double v = dl[i];
                for (int k = 0; k < i; k++) v -= Lu[i * ENKF_OBS + k] * w[k];
                w[i] = v / Lu[i * ENKF_OBS + i];
                logdet += log(Lu[i * ENKF_OBS + i]);
                q += w[i] * w[i];
            }
            ll = -0.5 * ((double)W * log(2.0 * M_PI) + 2.0 * logdet + q);
        }
        if (stats) {
            double *st = stats + ((size_t)p * n_arow + slot) * ENKF_WIDTH;
            st[0] = (double)mpp;
            st[1] = yb[0];
            st[2] = sqrt(cyy[0]);
            st[3] = dl[0];
            st[4] = ll;
        }
        if (stats && s.ms > 0) {
            double *ss = sm_stats + ((size_t)p * n_arow + slot) * s.n * ENKF_SENSOR_WIDTH;
            for (int i = 0; i < s.n; i++) ss[i * ENKF_SENSOR_WIDTH] = 0.0;      // observed: 0 unless present (the rest stays NaN)
            for (int k = 0; k < s.ms; k++) {
                double *e = ss + s.sensor[k] * ENKF_SENSOR_WIDTH;
                e[0] = 1.0;
                e[1] = s.obs[k];
                e[2] = yb[k + 1];
                e[3] = sqrt(cyy[(k + 1) * ENKF_OBS + k + 1]);
            }
        }
        if (stats && s.m > s.ms) {
            double *ws = win_stats + ((size_t)p * n_arow + slot) * s.nw * ENKF_WINDOW_WIDTH;
            for (int i = 0; i < s.nw; i++) ws[i * ENKF_WINDOW_WIDTH] = 0.0;     // observed: 0 unless present (the rest stays NaN)
            for (int k = s.ms; k < s.m; k++) {
                double *e = ws + s.sensor[k] * ENKF_WINDOW_WIDTH;
                e[0] = 1.0;
                e[1] = s.obs[k];
                e[2] = yb[k + 1];
                e[3] = sqrt(cyy[(k + 1) * ENKF_OBS + k + 1]);
            }
        }
    }
    __syncthreads();
    const int d = threadIdx.x;
    if (d >= D) return;
    double *K = gain + (size_t)p * W * D + d;
    double *Kr = rgain ? rgain + (size_t)p * W * D + d : nullptr;
    if (!ok) {
        for (int i = 0; i < W; i++) K[(size_t)i * D] = __builtin_nan("");
        if (Kr) {
            for (int i = 0; i < W; i++) Kr[(size_t)i * D] = __builtin_nan("");
            dbar[(size_t)p * D + d] = __builtin_nan("");
        }
        return;
    }
    double *u = U[d];
    for (int i = 0; i < W; i++) {
        const double rho = loc > 0.0 && taper_x ? gaspari_cohn(fabs((double)d * dz - zeta[i]) / loc) : 1.0;
        double v = rho * (mpp > 1 ? S2[(size_t)d * W + i] / n1 : 0.0);
        for (int k = 0; k < i; k++) v -= Ls[i * ENKF_OBS + k] * u[k];
        u[i] = v / Ls[i * ENKF_OBS + i];
    }
    for (int i = W - 1; i >= 0; i--) {
        double v = u[i];
        for (int k = i + 1; k < W; k++) v -= Ls[k * ENKF_OBS + i] * u[k];
        u[i] = v / Ls[i * ENKF_OBS + i];
    }
    for (int i = 0; i < W; i++) K[(size_t)i * D] = u[i];
    if (!Kr) return;
    double inc = 0.0;
    for (int i = 0; i < W; i++) inc += u[i] * dl[i];
    dbar[(size_t)p * D + d] = inc;
    for (int i = 0; i < W; i++) {
        const double rho = loc > 0.0 && taper_x ? gaspari_cohn(fabs((double)d * dz - zeta[i]) / loc) : 1.0;
        double v = rho * (mpp > 1 ? S2[(size_t)d * W + i] / n1 : 0.0);
        for (int k = 0; k < i; k++) v -= Ls[i * ENKF_OBS + k] * u[k];
        u[i] = v / Ls[i * ENKF_OBS + i];
    }
    // x (L + R^1/2) = u: x_i = (u_i - sum_{k > i} (L + R^1/2)_ki x_k) / (L_ii + r_i), r_i = sqrt(r2_i) (off the diagonal
    // L + R^1/2 is L)
    for (int i = W - 1; i >= 0; i--) {
        double v = u[i];
        for (int k = i + 1; k < W; k++) v -= Ls[k * ENKF_OBS + i] * u[k];
        u[i] = v / (Ls[i * ENKF_OBS + i] + sqrt(r2[i]));
    }
    for (int i = 0; i < W; i++) Kr[(size_t)i * D] = u[i];
}

// lane i's v, for every lane of the wave, in scalar registers (v_readlane reads lane i whichever lanes are active)
__device__ __forceinline__ double lane_value(double v, int i)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), i);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// eps_k of every member, and sensor i's (i < n) into eps_s [N][n] (one thread per member)
__global__ void enkf_draw_kernel(long long n_members, long long mpp, unsigned long long seed, const long long *point_base,
                                 long long member_offset, unsigned row, int n, double *eps, double *eps_s)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const unsigned long long gid = point_base ? (unsigned long long)(point_base[m / mpp] + m % mpp)
                                              : (unsigned long long)(member_offset + m);
    eps[m] = enkf_normal_at(0xFFFFFFFEu, seed, gid, row);
    for (int i = 0; i < n; i++) eps_s[(size_t)m * n + i] = enkf_normal_at(0xFFFFFFF0u + (unsigned)i, seed, gid, row);
}

// eps of the lagged columns, [N][m_w] in column order: the well's own normal with the lagged row in the row word -- the
// draw the well would have had on that row, which is never an analysis row (an offset is below the stride)
__global__ void enkf_window_draw_kernel(long long n_members, long long mpp, unsigned long long seed,
                                        const long long *point_base, long long member_offset, const EnkfRow s,
                                        double *eps_w)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const unsigned long long gid = point_base ? (unsigned long long)(point_base[m / mpp] + m % mpp)
                                              : (unsigned long long)(member_offset + m);
    const int mw = s.m - s.ms;
    for (int k = 0; k < mw; k++) eps_w[(size_t)m * mw + k] = enkf_normal_at(0xFFFFFFFEu, seed, gid, s.wrow[s.ms + k]);
}

// ---- one wave per member: the update of either scheme and the relaxation to prior spread
// A wave holds a member's column in a (node c * WAVE + lane in a[c], 0 past D).
// enkf_keep_column: `next` is stored and becomes a when every entry of it is finite (the wave's vote); else a stays.
// (The branch on the wave-uniform keep goes around the slot loop: one inside it costs 16 VGPRs of copies and a wave of
// occupancy.)
__device__ __forceinline__ bool enkf_keep_column(double (&a)[ENKF_SLOTS], const double (&next)[ENKF_SLOTS], double *col,
                                                 int lane, int D)
{
    bool ok = true;
#pragma unroll
    for (int c = 0; c < ENKF_SLOTS; c++) ok = ok && isfinite(next[c]);
    const bool keep = __all(ok);
    if (keep) {
#pragma unroll
        for (int c = 0; c < ENKF_SLOTS; c++) {
            const int d = c * WAVE + lane;
            a[c] = next[c];
            if (d < D) col[d] = next[c];
        }
    }
    return keep;
}

// enkf_column_y: find_wtd of the column (the step kernel's rule: below the deepest node with psi < psi_sat, clamped)
// and its y, on every lane
__device__ __forceinline__ double enkf_column_y(const double (&a)[ENKF_SLOTS], int lane, int D, double psat, double dz)
{
    int deepest = -1;
#pragma unroll
    for (int c = 0; c < ENKF_SLOTS; c++) {
        const int d = c * WAVE + lane;
        const unsigned long long u = __ballot(d < D && !(a[c] >= psat));
        if (u) deepest = c * WAVE + 63 - __clzll((long long)u);
    }
    const int b = deepest < 0 ? 0 : (deepest + 1 < D - 1 ? deepest + 1 : D - 1);
    const int bl = b >= 1 ? b - 1 : 0;
    double hi = 0.0, lo = 0.0;
#pragma unroll
    for (int c = 0; c < ENKF_SLOTS; c++) {
        const double x = __shfl(a[c], b % WAVE), xl = __shfl(a[c], bl % WAVE);
        if (c == b / WAVE) hi = x;
        if (c == bl / WAVE) lo = xl;
    }
    return enkf_y_of(b, lo, hi, psat, dz);
}

// The update of both schemes for the wave's member: psi_d + inc_d on every node of its column col, where inc = start +
// sum_{i >= 1} K_id dl_i summed in i order, one row of the point's gain K [W][D] at a time with the loads of all its
// slots in flight; lane i holds dl_i in my_dl, and start is K_0d dl_0, or with SHIFT shift_d + K_0d dl_0.
// Invariant of the padding: a slot past D holds 0.0 in a and in the candidate column, so the vote and find_wtd are
// decided by the nodes below D alone.  psi_d + inc_d is therefore formed below D only; past D inc is a sum of 0 * dl_i,
// which is NaN when an innovation is not finite.  Such an innovation also makes every node below D non-finite (K_id dl_i
// is then inf or NaN for every d), so the member is rejected whether or not the padding is looked at.  The column is
// stored only when every entry is finite (else the forecast stays and the member is counted as rejected); then the
// find_wtd index and the y of the column it kept: out = Ypost[m] = (y, ..., rejected), V entries (enkf_theta_kernel
// fills in the posterior theta).  want_y = 0: the relaxation follows and writes y.
// STATE = false: col is the member's base noise vector (hc_set_enkf_noise_field), which has no water table: the vote
// stays, the tail does not, and out[0] = 1.0 when the vector was refused, else 0.0.
template <bool SHIFT, bool STATE>
__device__ __forceinline__ void enkf_update_column(double *col, const double *K, const double *shift, int W, double my_dl,
                                                   int lane, int D, double psat, double dz, int want_y, double *out, int V)
{
#pragma clang fp contract(off)
    double a[ENKF_SLOTS], inc[ENKF_SLOTS], k0[ENKF_SLOTS];
#pragma unroll
    for (int c = 0; c < ENKF_SLOTS; c++) {
        const int d = c * WAVE + lane;
        a[c] = 0.0;
        inc[c] = 0.0;
        k0[c] = 0.0;
        if (d < D) {
            a[c] = col[d];
            if (SHIFT) inc[c] = shift[d];
            k0[c] = K[d];
        }
    }
    const double dl0 = lane_value(my_dl, 0);
#pragma unroll
    for (int c = 0; c < ENKF_SLOTS; c++) inc[c] = SHIFT ? inc[c] + k0[c] * dl0 : k0[c] * dl0;
#pragma unroll 1
    for (int i = 1; i < W; i++) {
        const double di = lane_value(my_dl, i);
        double k[ENKF_SLOTS];
#pragma unroll
        for (int c = 0; c < ENKF_SLOTS; c++) {
            const int d = c * WAVE + lane;
            k[c] = d < D ? K[(size_t)i * D + d] : 0.0;
        }
#pragma unroll
        for (int c = 0; c < ENKF_SLOTS; c++) inc[c] = inc[c] + k[c] * di;
    }
#pragma unroll
    for (int c = 0; c < ENKF_SLOTS; c++) inc[c] = c * WAVE + lane < D ? a[c] + inc[c] : 0.0;
    const bool keep = enkf_keep_column(a, inc, col, lane, D);
    if (!STATE) {
        if (lane == 0) out[0] = keep ? 0.0 : 1.0;
        return;
    }
    if (want_y) {
        const double y = enkf_column_y(a, lane, D, psat, dz);
        if (lane == 0) out[0] = y;
    }
    if (lane == 0) out[V - 1] = keep ? 0.0 : 1.0;
}

// The stochastic update, one wave per member: lane i's innovation is o_i + sigma_i eps_ki - Y_ki from the draws of
// enkf_draw_kernel (and enkf_window_draw_kernel): the well's on lane 0, present sensor k's and then the lagged rows' on
// lane 1 + k.
// STATE = false updates the members' base noise vectors (psi = the base array, gain = their gain) after the state's
// update, with the same innovations: a member whose state was refused (Ypost[m][V - 1] != 0) keeps its vector to the
// bit, and refused[m] = 1.0 for a member whose updated vector was not finite (it keeps the old one), else 0.0.
template <bool STATE>
__global__ __launch_bounds__(256) void enkf_update_kernel(double *psi, const double *Y, const double *gain,
                                                          const ColumnDev *P, long long n_members, long long mpp, int D,
                                                          double dz, double z_obs, double sigma, const EnkfRow s,
                                                          const double *eps, const double *eps_s,
                                                          const double *eps_w, int want_y, double *Ypost, double *refused)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x % WAVE;
    const int W = s.m + 1, V = s.ms + 2, mw = s.m - s.ms;
    // lane 1 + k holds column k beyond the well's: present sensor k's record index, observation and sigma; a lagged
    // row's (k >= ms) place among the lagged columns instead of the index
    int my_sensor = 0;
    double my_obs = 0.0, my_sigma = 0.0;
#pragma unroll
    for (int k = 0; k < ENKF_SENSORS; k++)
        if (k < s.m && lane == 1 + k) my_sensor = k < s.ms ? s.sensor[k] : k - s.ms, my_obs = s.obs[k], my_sigma = s.sigma[k];
    const long long waves = (long long)gridDim.x * (blockDim.x / WAVE);
    for (long long m = (long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; m < n_members; m += waves) {
        const long long p = m / mpp;
        const double *Ym = Y + (size_t)m * W;
        const double my_dl = lane == 0      ? (z_obs + sigma * eps[m]) - Ym[0]
                             : lane <= s.ms ? (my_obs + my_sigma * eps_s[(size_t)m * s.n + my_sensor]) - Ym[lane]
                             : lane < W     ? (my_obs + my_sigma * eps_w[(size_t)m * mw + my_sensor]) - Ym[lane]
                                            : 0.0;
        if (!STATE && Ypost[(size_t)m * V + V - 1] != 0.0) {
            if (lane == 0) refused[m] = 0.0;
            continue;
        }
        enkf_update_column<false, STATE>(psi + (size_t)m * D, gain + (size_t)p * W * D, nullptr, W, my_dl, lane, D,
                                         P[p].psi_sat, dz, want_y, STATE ? Ypost + (size_t)m * V : refused + m, V);
    }
}

// The square-root update (Whitaker & Hamill 2002), one wave per member: the reduced gain, the mean's increment dbar as
// the shift, and lane i's innovation Ybar_i - Y_ki (Ybar from the prior sums s1 [P][D + m']).  Nothing is drawn.
// STATE = false: the base noise vectors, as in enkf_update_kernel.
template <bool STATE>
__global__ __launch_bounds__(256) void enkf_sqrt_update_kernel(double *psi, const double *Y, const double *rgain,
                                                               const double *dbar, const double *s1, const ColumnDev *P,
                                                               long long n_members, long long mpp, int D, double dz,
                                                               int W, int V, int want_y, double *Ypost, double *refused)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x % WAVE;
    const long long waves = (long long)gridDim.x * (blockDim.x / WAVE);
    for (long long m = (long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; m < n_members; m += waves) {
        const long long p = m / mpp;
        const double my_dl = lane < W ? s1[(size_t)p * (D + W) + D + lane] / (double)mpp - Y[(size_t)m * W + lane] : 0.0;
        if (!STATE && Ypost[(size_t)m * V + V - 1] != 0.0) {
            if (lane == 0) refused[m] = 0.0;
            continue;
        }
        enkf_update_column<true, STATE>(psi + (size_t)m * D, rgain + (size_t)p * W * D, dbar + (size_t)p * D, W, my_dl, lane,
                                        D, P[p].psi_sat, dz, want_y, STATE ? Ypost + (size_t)m * V : refused + m, V);
    }
}

// The spread of the analysis columns, thread d = node d, by the tile rule of enkf_partial_kernel (its mpp, np, tile0
// and to = tile0 + t).  The columns are taken relative to the point's first member, x = psi_d - psi_d[member 0]:
//   sums == NULL: partial[p][to][d] = sum over the tile in member order of x;
//   otherwise:    partial[p][to][d] = sum of (x - xbar)^2, xbar = sums[p][d] / np.
// So a node on which every member agrees (a saturated tail) has x = 0, the mean psi_d[member 0] and sigma_a = 0 exactly,
// where the plain sum of N equal values rounds.  Point p's first member's column is first + p * first_stride: psi and
// mpp * D, or the copy another handle contributed and 0 (hc_set_enkf_shard).
__global__ __launch_bounds__(HC_MAX_DEPTH_NODES) void enkf_spread_kernel(const double *psi, const double *sums,
                                                                         long long mpp, int D, long long n_tiles,
                                                                         double *partial, const double *first,
                                                                         long long first_stride, long long np,
                                                                         long long tile0)
{
#pragma clang fp contract(off)
    const long long p = blockIdx.y, t = blockIdx.x;
    const int d = threadIdx.x;
    if (d >= D) return;
    const long long m0 = p * mpp + t * ENKF_TILE;
    const long long m1 = p * mpp + ((t + 1) * ENKF_TILE < mpp ? (t + 1) * ENKF_TILE : mpp);
    const double *x = psi + d;
    const double x0 = first[(size_t)(p * first_stride) + d];
    double s = 0.0;
    if (!sums) {
#pragma unroll 8
        for (long long m = m0; m < m1; m++) s += x[(size_t)m * D] - x0;
    } else {
        const double xb = sums[(size_t)p * D + d] / (double)np;
#pragma unroll 8
        for (long long m = m0; m < m1; m++) {
            const double a = (x[(size_t)m * D] - x0) - xb;
            s += a * a;
        }
    }
    partial[((size_t)p * n_tiles + tile0 + t) * D + d] = s;
}

// the point's first member's column, by the handle that holds it, into the exchange buffer (hc_set_enkf_shard)
__global__ void enkf_first_member_kernel(const double *psi, int D, double *first)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < D) first[d] = psi[d];
}

// Relaxation to prior spread (Whitaker & Hamill 2012), one thread per point and node: from the sums of the squared psi
// anomalies before and after the update, sigma_b, sigma_a (N_p - 1; N_p = 1: 0) and f = 1 + alpha (sigma_b - sigma_a) /
// sigma_a; f = 1 where sigma_a is 0 or not finite and for a point whose factorisation failed (a NaN gain); the mean of
// the analysis, psi_d[member 0] + sums / N_p (enkf_spread_kernel).  relax = (sigma_b, sigma_a, f, mean), [P][D] each.
__global__ void enkf_relax_factor_kernel(const double *sq_b, const double *sq_a, const double *sums, const double *psi,
                                         const double *gain, long long n_points, long long mpp, int D, int W, double alpha,
                                         double *relax)
{
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = n_points * D;
    if (k >= n) return;
    const long long p = k / D;
    const double n1 = (double)(mpp - 1);
    const double sb = mpp > 1 ? sqrt(sq_b[k] / n1) : 0.0, sa = mpp > 1 ? sqrt(sq_a[k] / n1) : 0.0;
    double f = 1.0;
    if (sa > 0.0 && isfinite(sa) && isfinite(gain[(size_t)p * W * D])) f = 1.0 + alpha * (sb - sa) / sa;
    relax[k] = sb;
    relax[n + k] = sa;
    relax[2 * n + k] = f;
    relax[3 * n + k] = psi[(size_t)(p * mpp) * D + k % D] + sums[k] / (double)mpp;
}

// One wave per member: psi_dk <- mean_d + f_d (psi_dk - mean_d) (the analysis's mean [P][D]; a node with f_d = 1
// stays as it is), stored only when every entry is finite (else the member keeps its unrelaxed analysis); then find_wtd
// and y of the column it kept into Ypost[m][0] (rows of `width` entries).  STATE = false: the base noise vectors; no y,
// and a member whose state's analysis was refused (Ypost[m][width - 1] != 0), or whose own updated vector was
// (refused[m] != 0), is left alone.
template <bool STATE>
__global__ __launch_bounds__(256) void enkf_relax_kernel(double *psi, const double *means, const double *factor,
                                                         const ColumnDev *P, long long n_members, long long mpp, int D,
                                                         double dz, int width, double *Ypost, const double *refused)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x % WAVE;
    const long long waves = (long long)gridDim.x * (blockDim.x / WAVE);
    for (long long m = (long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; m < n_members; m += waves) {
        const long long p = m / mpp;
        if (!STATE && (Ypost[(size_t)m * width + width - 1] != 0.0 || refused[m] != 0.0)) continue;
        const double *S = means + (size_t)p * D, *F = factor + (size_t)p * D;
        double *col = psi + (size_t)m * D;
        double a[ENKF_SLOTS], r[ENKF_SLOTS];
#pragma unroll
        for (int c = 0; c < ENKF_SLOTS; c++) {
            const int d = c * WAVE + lane;
            a[c] = 0.0;
            r[c] = 0.0;
            if (d < D) {
                const double mean = S[d], f = F[d];
                a[c] = col[d];
                r[c] = f == 1.0 ? a[c] : mean + f * (a[c] - mean);
            }
        }
        enkf_keep_column(a, r, col, lane, D);
        if (STATE) {
            const double y = enkf_column_y(a, lane, D, P[p].psi_sat, dz);
            if (lane == 0) Ypost[(size_t)m * width] = y;
        }
    }
}

// The noise field's diagnostics, one thread per point and node: the prior mean and std of z_d from the prior sums
// (s1 [P][D + m'], the squared anomalies sq_b), the posterior's -- after the relaxation -- from the spread passes (z_d of
// the point's first member + sums / N_p; sq_a), into table[p][slot][4][D]; node 0's thread adds the point's refused
// count behind them.
__global__ void enkf_noise_diag_kernel(const double *s1, const double *sq_b, const double *sums, const double *sq_a,
                                       const double *base, const double *rejsum, long long n_points, long long mpp, int D,
                                       int W, double *table, long long n_arow, long long slot)
{
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_points * D) return;
    const long long p = k / D;
    const int d = (int)(k % D);
    const double n1 = (double)(mpp - 1);
    double *t = table + ((size_t)p * n_arow + slot) * (4 * (size_t)D + 1);
    t[d] = s1[(size_t)p * (D + W) + d] / (double)mpp;
    t[D + d] = mpp > 1 ? sqrt(sq_b[k] / n1) : 0.0;
    t[2 * D + d] = base[(size_t)(p * mpp) * D + d] + sums[k] / (double)mpp;
    t[3 * D + d] = mpp > 1 ? sqrt(sq_a[k] / n1) : 0.0;
    if (d == 0) t[4 * (size_t)D] = rejsum[p];
}

// ---- the members' forcing state in the analysis (hc_set_enkf_forcing): g [2][N] is stream-major, the analysis's kernels
// walk member-major columns, so g goes through x [N][2] and back (one thread per member; a copy keeps every bit)
__global__ void enkf_forcing_gather_kernel(const double *g, long long n_members, double *x)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    x[2 * (size_t)m] = g[m];
    x[2 * (size_t)m + 1] = g[(size_t)n_members + m];
}

// ... and back, the streams that are analysed alone (active_s = sigma_s > 0): the other keeps every bit of its g
__global__ void enkf_forcing_scatter_kernel(const double *x, long long n_members, int active0, int active1, double *g)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    if (active0) g[m] = x[2 * (size_t)m];
    if (active1) g[(size_t)n_members + m] = x[2 * (size_t)m + 1];
}

// The forcing state's diagnostics, one thread per point and stream, into table[p][slot][9]: columns 4 s + (prior mean,
// prior std, posterior mean, posterior std) as enkf_noise_diag_kernel forms them from the prior sums (s1 [P][2 + m'],
// sq_b) and the spread passes after the relaxation (x of the point's first member + sums / N_p; sq_a); a stream that is
// not analysed reports its prior twice; stream 0's thread adds the point's refused count in column 8.
__global__ void enkf_forcing_diag_kernel(const double *s1, const double *sq_b, const double *sums, const double *sq_a,
                                         const double *x, const double *rejsum, long long n_points, long long mpp, int W,
                                         int active0, int active1, double *table, long long n_arow, long long slot)
{
#pragma clang fp contract(off)
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_points * 2) return;
    const long long p = k / 2;
    const int s = (int)(k % 2);
    const double n1 = (double)(mpp - 1);
    double *t = table + ((size_t)p * n_arow + slot) * ENKF_FORCING_WIDTH;
    const double mean_b = s1[(size_t)p * (2 + W) + s] / (double)mpp, std_b = mpp > 1 ? sqrt(sq_b[k] / n1) : 0.0;
    const bool active = s ? active1 != 0 : active0 != 0;
    t[4 * s] = mean_b;
    t[4 * s + 1] = std_b;
    t[4 * s + 2] = active ? x[(size_t)(p * mpp) * 2 + s] + sums[k] / (double)mpp : mean_b;
    t[4 * s + 3] = active ? (mpp > 1 ? sqrt(sq_a[k] / n1) : 0.0) : std_b;
    if (s == 0) t[8] = rejsum[p];
}

// One thread per point: the posterior diagnostics from the raw sums of Ypost (s1 [P][W + 1], s2 [P][W + 1][W + 1]): the
// EnKF's entries 5-7 and the sensors' posterior mean and std.
__global__ void enkf_post_kernel(const double *s1, const double *s2, long long n_points, long long mpp, const EnkfRow s,
                                 double *stats, double *sm_stats, long long n_arow, long long slot)
{
#pragma clang fp contract(off)
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_points) return;
    const int V = s.ms + 2;
    const double *S1 = s1 + (size_t)p * V, *S2 = s2 + (size_t)p * V * V;
    const double n1 = (double)(mpp - 1);
    double *st = stats + ((size_t)p * n_arow + slot) * ENKF_WIDTH;
    st[5] = S1[0] / (double)mpp;
    st[6] = sqrt(mpp > 1 ? S2[0] / n1 : 0.0);
    st[7] = S1[V - 1];
    for (int k = 0; k < s.ms; k++) {
        double *e = sm_stats + (((size_t)p * n_arow + slot) * s.n + s.sensor[k]) * ENKF_SENSOR_WIDTH;
        e[4] = S1[k + 1] / (double)mpp;
        e[5] = sqrt(mpp > 1 ? S2[(size_t)(k + 1) * V + k + 1] / n1 : 0.0);
    }
}

// ---- soil-moisture sensors in the particle filter (hc_set_filter_soil_moisture, include/hydrocol.h)
// A row with sensor values weighs every member by itself.  Y [N][m_s + 2] holds per member l_m, theta at the nodes of the
// present sensors (enkf_theta_kernel writes columns 1 ... m_s) and e_m = exp(l_m - s).  A block is one tile of the prefix
// scan: FILT_THREADS threads with FILT_PER_THREAD consecutive members each.  Every floating-point sum over a point's
// members runs in the one order of filter_tile_partial_kernel and filter_column_sum -- fixed by N_p alone, no
// floating-point atomics; maxima and integer sums do not depend on an order.  Contraction is off throughout.
constexpr int FILT_COLS = ENKF_SENSORS + 1;            // the columns summed: theta of the present sensors, then e

// the largest v of the block's threads (every thread gets it)
__device__ double filter_block_max(double v)
{
    __shared__ double sh[FILT_THREADS];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = FILT_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = sh[threadIdx.x + o] > sh[threadIdx.x] ? sh[threadIdx.x + o] : sh[threadIdx.x];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// a member is counted when its water table lies in the column and its log-likelihood is finite
__device__ __forceinline__ bool filter_counted(int b, int D, double l) { return b < D && isfinite(l); }

// Y[m][0] = l_m = -0.5 (t_w^2 + sum over the present sensors, in record order, of ((theta_m,i - theta_obs,i) / sigma_i)^2)
// with the well's t_w = dz (b_m - o) / sigma_cm; lmax[p][t] = the largest l_m of the tile's counted members (-inf: none).
// hc_set_filter_window: the present lagged rows follow the sensors by ascending offset, column i >= ms with the member's
// index b_m(r_j) = lag[slot][m] of that row (window_capture_kernel) and the row's observed index s.node[i]:
// t_j = dz (b_m(r_j) - o_j) / sigma_cm, a += t_j^2, and Y[m][1 + i] = dz b_m(r_j), the lagged depth the diagnostics sum.
// wmax[m] = the largest of the member's indices (lagged columns only): it is counted when every one lies in the column.
__global__ __launch_bounds__(FILT_THREADS) void filter_loglik_kernel(const unsigned short *w, long long members_per_point,
                                                                     int D, int obs, double dz, double sigma,
                                                                     const EnkfRow s, double *Y, long long n_tiles,
                                                                     double *lmax, const int *lag, long long n_members,
                                                                     unsigned short *wmax)
{
#pragma clang fp contract(off)
    const long long p = blockIdx.y, t = blockIdx.x;
    const int width = s.m + 2;
    double best = -INFINITY;
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = t * FILT_TILE + (long long)threadIdx.x * FILT_PER_THREAD + j;
        if (m >= members_per_point) continue;
        const size_t k = (size_t)(p * members_per_point + m);
        int b = (int)w[k];
        double *y = Y + k * width;
        const double tw = dz * (double)(b - obs) / sigma;
        double a = tw * tw;
        for (int i = 0; i < s.ms; i++) {
            const double u = (y[1 + i] - s.obs[i]) / s.sigma[i];
            a += u * u;
        }
        for (int i = s.ms; i < s.m; i++) {
            const int bj = lag[(size_t)s.sensor[i] * n_members + k];
            const double tj = dz * (double)(bj - s.node[i]) / sigma;
            a += tj * tj;
            y[1 + i] = dz * (double)bj;
            b = bj > b ? bj : b;
        }
        const double l = -0.5 * a;
        y[0] = l;
        if (s.m > s.ms) wmax[k] = (unsigned short)b;
        if (filter_counted(b, D, l)) best = l > best ? l : best;
    }
    best = filter_block_max(best);
    if (threadIdx.x == 0) lmax[(size_t)p * n_tiles + t] = best;
}

// s = the largest lmax[p][.]; per member e_m = exp(l_m - s) -> Y[m][ms + 1] and q_m = floor(2^31 e_m) -> qm[m] (0 and 0
// for a member that is not counted); ipart[p][t] = the tile's {sum q, sum q^2 low word, high word, members counted};
// smax[p] = s.  (ms: the columns between l and e -- the present sensors and, hc_set_filter_window, the lagged rows; w is
// then the members' largest indices)
__global__ __launch_bounds__(FILT_THREADS) void filter_member_weights_kernel(const unsigned short *w,
                                                                             long long members_per_point, int D, int ms,
                                                                             long long n_tiles, const double *lmax,
                                                                             double *Y, long long *qm,
                                                                             unsigned long long *ipart, double *smax)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long part[FILT_THREADS / WAVE][4];
    const long long p = blockIdx.y, t = blockIdx.x;
    const int width = ms + 2;
    double s = -INFINITY;
    for (long long u = threadIdx.x; u < n_tiles; u += FILT_THREADS) {
        const double v = lmax[(size_t)p * n_tiles + u];
        s = v > s ? v : s;
    }
    s = filter_block_max(s);
    unsigned long long Q = 0, hi = 0, lo = 0, n = 0;
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = t * FILT_TILE + (long long)threadIdx.x * FILT_PER_THREAD + j;
        if (m >= members_per_point) continue;
        const size_t k = (size_t)(p * members_per_point + m);
        double *y = Y + k * width;
        double e = 0.0;
        long long q = 0;
        if (filter_counted((int)w[k], D, y[0])) {
            e = exp(y[0] - s);
            q = (long long)floor(0x1p31 * e);                  // 2^31 at the likeliest member, 0 below ~2^-31
            n++;
        }
        y[ms + 1] = e;
        qm[k] = q;
        const unsigned long long uq = (unsigned long long)q;
        Q += uq;                                               // < 2^31 members x 2^31
        add_u128(hi, lo, 0ull, uq * uq);                       // each < 2^62
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long ohi = __shfl_xor(hi, o), olo = __shfl_xor(lo, o);
        add_u128(hi, lo, ohi, olo);
        Q += __shfl_xor(Q, o);
        n += __shfl_xor(n, o);
    }
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (lane == 0) {
        part[wave][0] = Q;
        part[wave][1] = lo;
        part[wave][2] = hi;
        part[wave][3] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Q = n = hi = lo = 0;
        for (int u = 0; u < FILT_THREADS / WAVE; u++) {
            Q += part[u][0];
            add_u128(hi, lo, part[u][2], part[u][1]);
            n += part[u][3];
        }
        unsigned long long *out = ipart + ((size_t)p * n_tiles + t) * 4;
        out[0] = Q;
        out[1] = lo;
        out[2] = hi;
        out[3] = n;
        if (t == 0) smax[p] = s;
    }
}

// partial[p][t][c] = the sum over tile t of point p of f(Y[src][col0 + c]), c < n_cols.  src = the member itself, or (anc)
// the ancestor of the slot; f(x) = x, or (mean) (x - mean[p][c])^2.  The order: every thread its FILT_PER_THREAD
// consecutive members, in member order from 0.0; then the block's FILT_THREADS threads in a tree of halving strides
// (thread i takes thread i + 128's, then i + 64's, ...).  Members past the point's end add 0.0.
__global__ __launch_bounds__(FILT_THREADS) void filter_tile_partial_kernel(const double *Y, int width, int col0, int n_cols,
                                                                           const long long *anc, const double *mean,
                                                                           long long members_per_point, long long n_members,
                                                                           long long n_tiles, double *partial)
{
#pragma clang fp contract(off)
    __shared__ double sh[FILT_THREADS];
    const long long p = blockIdx.y, t = blockIdx.x;
    long long src[FILT_PER_THREAD];
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = t * FILT_TILE + (long long)threadIdx.x * FILT_PER_THREAD + j;
        src[j] = -1;
        if (m < members_per_point) {
            const long long k = p * members_per_point + m, a = anc ? anc[k] : k;
            src[j] = a >= 0 && a < n_members ? a : k;          // (every slot is filled: a guard)
        }
    }
    for (int c = 0; c < n_cols; c++) {
        const double mu = mean ? mean[(size_t)p * FILT_COLS + c] : 0.0;
        double v = 0.0;
        for (int j = 0; j < FILT_PER_THREAD; j++) {
            if (src[j] < 0) continue;
            const double x = Y[(size_t)src[j] * width + col0 + c];
            if (mean) {
                const double d = x - mu;
                v += d * d;
            } else {
                v += x;
            }
        }
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = FILT_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[((size_t)p * n_tiles + t) * n_cols + c] = sh[0];
        __syncthreads();
    }
}

// column c's tile partials of point p, tiles ascending from 0.0
__device__ __forceinline__ double filter_column_sum(const double *partial, long long p, long long n_tiles, int n_cols, int c)
{
#pragma clang fp contract(off)
    double v = 0.0;
    for (long long t = 0; t < n_tiles; t++) v += partial[((size_t)p * n_tiles + t) * n_cols + c];
    return v;
}

// One block per point after the weights, the partials being those of (theta of the present sensors, the depths of the
// present lagged rows, e).  Thread c < ms: sensor c's observed, observation and forecast mean (also -> mean[p][c]); a
// thread per absent sensor of the record: observed = 0, the rest NaN; thread ms <= c < m: the same for lagged column c in
// the window's table, and a thread per absent offset; thread 0: W, the exact integer sums, the filter's count, ESS and
// increment, and the draw.
__global__ void filter_member_finish_kernel(const double *partial, const unsigned long long *ipart, const double *smax,
                                            long long n_tiles, long long members_per_point, const EnkfRow s, double sigma,
                                            unsigned long long seed, const long long *point_base, long long member_offset,
                                            unsigned row, long long n_arow, long long slot, unsigned long long *qr,
                                            double *stats, unsigned long long *surv, double *mean, double *sm_stats,
                                            double *win_stats)
{
#pragma clang fp contract(off)
    const long long p = blockIdx.x;
    const int c = threadIdx.x, n_cols = s.m + 1;
    double *sm = sm_stats + ((size_t)p * n_arow + slot) * s.n * ENKF_SENSOR_WIDTH;
    double *wn = win_stats + ((size_t)p * n_arow + slot) * s.nw * ENKF_WINDOW_WIDTH;
    if (c < s.m) {
        const double mu = filter_column_sum(partial, p, n_tiles, n_cols, c) / (double)members_per_point;
        mean[(size_t)p * FILT_COLS + c] = mu;
        double *e = c < s.ms ? sm + (size_t)s.sensor[c] * ENKF_SENSOR_WIDTH : wn + (size_t)s.sensor[c] * ENKF_WINDOW_WIDTH;
        e[0] = 1.0;
        e[1] = s.obs[c];
        e[2] = mu;
    }
    if (c < s.n) {
        bool present = false;
        for (int k = 0; k < s.ms; k++) present = present || s.sensor[k] == c;
        if (!present) {
            double *e = sm + (size_t)c * ENKF_SENSOR_WIDTH;
            e[0] = 0.0;
            for (int k = 1; k < ENKF_SENSOR_WIDTH; k++) e[k] = __builtin_nan("");
        }
    }
    if (c < s.nw) {
        bool present = false;
        for (int k = s.ms; k < s.m; k++) present = present || s.sensor[k] == c;
        if (!present) {
            double *e = wn + (size_t)c * ENKF_WINDOW_WIDTH;
            e[0] = 0.0;
            for (int k = 1; k < ENKF_WINDOW_WIDTH; k++) e[k] = __builtin_nan("");
        }
    }
    if (c != 0) return;
    const double W = filter_column_sum(partial, p, n_tiles, n_cols, s.m);
    unsigned long long Q = 0, b_hi = 0, b_lo = 0, n = 0;
    for (long long t = 0; t < n_tiles; t++) {
        const unsigned long long *in = ipart + ((size_t)p * n_tiles + t) * 4;
        Q += in[0];
        add_u128(b_hi, b_lo, in[2], in[1]);
        n += in[3];
    }
    double *st = stats + ((size_t)p * n_arow + slot) * 4;
    st[0] = (double)n;
    if (n > 0 && Q > 0) {
        st[1] = filter_ess(Q, b_hi, b_lo);
        double inc = smax[p] + log(W / (double)n) - log(sigma);
        for (int k = 0; k < s.m; k++) inc -= log(s.sigma[k]);      // (a lagged column's is the well's sigma_cm)
        st[2] = inc - 0.5 * (double)(1 + s.m) * log(2.0 * M_PI);
    } else {
        st[1] = __builtin_nan("");
        st[2] = __builtin_nan("");
    }
    filter_draw(seed, point_base, member_offset, p, members_per_point, row, Q, qr, surv);
}

// One block per point, thread c < n_cols, from the partials of the first n_cols columns after l: entry = 4, the posterior
// mean (also -> mean[p][c]); entry = 3 or 5, a std from the squared deviations, / (N_p - 1) (N_p = 1: 0).  A column
// c >= ms is a lagged row's (hc_set_filter_window; entry 3 only): its forecast std goes to the window's table.
__global__ void filter_sm_moment_kernel(const double *partial, long long n_tiles, long long members_per_point,
                                        const EnkfRow s, int n_cols, int entry, long long n_arow, long long slot,
                                        double *mean, double *sm_stats, double *win_stats)
{
#pragma clang fp contract(off)
    const long long p = blockIdx.x;
    const int c = threadIdx.x;
    if (c >= n_cols) return;
    const double v = filter_column_sum(partial, p, n_tiles, n_cols, c);
    double *e = c < s.ms ? sm_stats + (((size_t)p * n_arow + slot) * s.n + s.sensor[c]) * ENKF_SENSOR_WIDTH
                         : win_stats + (((size_t)p * n_arow + slot) * s.nw + s.sensor[c]) * ENKF_WINDOW_WIDTH;
    if (entry == 4) {
        e[4] = mean[(size_t)p * FILT_COLS + c] = v / (double)members_per_point;
    } else {
        e[entry] = sqrt(members_per_point > 1 ? v / (double)(members_per_point - 1) : 0.0);
    }
}

// a bin-path row of a filter with a record: the per-member weights q_{b_m} (hc_get_filter_member_weights)
__global__ void filter_expand_weights_kernel(const unsigned short *w, const long long *q_all, long long members_per_point,
                                             long long n_members, int D, long long *qm)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_members) qm[k] = filter_q(w, q_all + (size_t)(k / members_per_point) * D, D, k);
}

// the lagged row a launch ended on (hc_set_filter_window): every member's water-table index of that row, widened, into the
// offset's row of the window's buffer [n_offsets][N]
__global__ void window_capture_kernel(const unsigned short *w, long long n_members, int *out)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_members) out[k] = (int)w[k];
}

// ---- fixed-lag smoother of the water table by ancestry (hc_set_filter_smoother, include/hydrocol.h): integers only
constexpr int SMO_PLANES = HC_SMOOTHER_MAX_LAG + 1;
// the ring's planes a gather moves: those that hold a row
struct SmootherPlanes {
    int n;
    unsigned char plane[SMO_PLANES];
};

// a record row into its plane: every member's water-table index of that row and, as the path's id, the member's index
// within its point
__global__ void smoother_store_kernel(const unsigned short *w, long long n_members, long long members_per_point,
                                      unsigned short *ring_w, unsigned *ring_id)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_members) {
        ring_w[k] = w[k];
        ring_id[k] = (unsigned)(k % members_per_point);
    }
}

// the particle filter's ancestry applied to the ring, next to period_gather_kernel: slot m takes its ancestor's values of
// every live plane (into the second buffers; the host swaps them in).  One thread per slot reads anc[m] once; each plane
// is read through it -- the ancestry of systematic resampling is non-decreasing within a point, so a wave's loads fall
// into a few lines -- and written coalesced.
__global__ __launch_bounds__(256) void smoother_gather_kernel(const long long *anc, long long n_members,
                                                              const SmootherPlanes L, const unsigned short *w,
                                                              const unsigned *id, unsigned short *w_out, unsigned *id_out)
{
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_members) return;
    const long long a = anc[m];
    const size_t src = (size_t)(a >= 0 && a < n_members ? a : m);     // (every slot is filled: a guard)
    for (int j = 0; j < L.n; j++) {
        const size_t at = (size_t)L.plane[j] * (size_t)n_members;
        w_out[at + (size_t)m] = w[at + src];
        id_out[at + (size_t)m] = id[at + src];
    }
}

// One plane into record slot `slot` of the tables: grid x = member slice, y = point.  The bins are counted as
// wtd_hist_kernel counts them (LDS, the wave's lanes grouped by bin with ballots first, int32 atomics of nonzero bins
// only; an index >= D goes to no bin).  The distinct paths: a store writes the identity and every ancestry is
// non-decreasing within a point, so the ids of a point's slots are non-decreasing and their distinct values number the
// slots that open a run -- the point's first slot and every slot whose id differs from its left neighbour's.  The left
// neighbour of a slice's first slot is read from the plane like any other (it lies in the same point); the point's first
// slot has none, and nothing at or past the slice's end is read.  One uint64 atomic per wave adds the count to
// spaths[point][slot][0]; the conditioning row goes to [1].
__global__ __launch_bounds__(HIST_THREADS) void smoother_emit_kernel(const unsigned short *w, const unsigned *id,
                                                                     long long members_per_point,
                                                                     long long members_per_block, long long n_srow,
                                                                     long long slot, long long cond_row, int D, int *shist,
                                                                     long long *spaths)
{
    __shared__ unsigned bins[HC_MAX_DEPTH_NODES];
    for (int b = threadIdx.x; b < D; b += HIST_THREADS) bins[b] = 0;
    __syncthreads();
    const long long point = blockIdx.y;
    const long long start = point * members_per_point, end = start + members_per_point;
    const long long m0 = start + (long long)blockIdx.x * members_per_block;
    const long long m1 = m0 + members_per_block < end ? m0 + members_per_block : end;
    const int lane = threadIdx.x % WAVE;
    unsigned long long heads = 0;
    // wave-uniform trip count: every lane of a wave runs the ballots of every round
    for (long long k0 = m0 + (threadIdx.x - lane); k0 < m1; k0 += HIST_THREADS) {
        const long long k = k0 + lane;
        const bool in = k < m1;
        const int b = in ? (int)w[k] : -1;
        const bool head = in && (k == start || id[k] != id[k - 1]);
        heads += (unsigned long long)__popcll(__ballot(head));
        unsigned long long pending = __ballot(b >= 0 && b < D);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int v = __builtin_amdgcn_readlane(b, leader);
            const unsigned long long same = __ballot(b == v) & pending;
            if (lane == leader) atomicAdd(&bins[v], (unsigned)__popcll(same));
            pending &= ~same;
        }
    }
    __syncthreads();
    int *t = shist + ((size_t)point * n_srow + (size_t)slot) * D;
    for (int b = threadIdx.x; b < D; b += HIST_THREADS) {
        const unsigned c = bins[b];
        if (c) atomicAdd(t + b, (int)c);
    }
    long long *p = spaths + ((size_t)point * n_srow + (size_t)slot) * 2;
    if (lane == 0 && heads) atomicAdd(reinterpret_cast<unsigned long long *>(p), heads);
    if (blockIdx.x == 0 && threadIdx.x == 0) p[1] = cond_row;
}

// ---- tempered weights (hc_set_filter_tempering, include/hydrocol.h)
// After the weight kernels, per point: the largest k of a bisection over beta_k = k / 1024 for which the weights
// q = floor(2^31 exp(beta_k (l - s))) keep Q^2 >= T sum q^2.  Q, sum q^2 and the comparison are exact integers, so k
// depends on no order.  The only floating-point arithmetic is the exp of a weight and the ESS quotient of the table;
// contraction is off.
constexpr int TEMPER_STEPS = 1024;                     // beta_k = k / TEMPER_STEPS
constexpr int TEMPER_TRIALS = 11;                      // k = 1024, then ten halvings of [0, 1024]
constexpr int TEMPER_WIDTH = 4;                        // table entries per point and slot; words per trial of the hook
// a point's search on a sensor row, int64 words: the k of the next trial (the result once done), lo, hi, done (2: the row
// is not tempered for want of members), trials evaluated, T, then Q and sum q^2 (low, high word) at lo
constexpr int TEMPER_STATE = 9;

// T = min(n, max(1, ceil(f n)))
__device__ __forceinline__ long long temper_target(double f, long long n)
{
#pragma clang fp contract(off)
    long long T = (long long)ceil(f * (double)n);
    T = T < 1 ? 1 : T;
    return T < n ? T : n;
}

// q at beta_k of a counted member or an occupied bin, d = l - s: the product rounded once; k = 1024 multiplies by 1.0
__device__ __forceinline__ long long temper_q(int k, double d)
{
#pragma clang fp contract(off)
    const double beta = (double)k / (double)TEMPER_STEPS;
    const double a = beta * d;
    return (long long)floor(0x1p31 * exp(a));
}

// Q^2 >= T S, both sides exact: Q < 2^62, T < 2^31, S < 2^93
__device__ __forceinline__ bool temper_ok(unsigned long long Q, unsigned long long s_hi, unsigned long long s_lo, long long T)
{
    const unsigned __int128 S = ((unsigned __int128)s_hi << 64) | s_lo;
    return (unsigned __int128)Q * Q >= (unsigned __int128)(unsigned long long)T * S;
}

// the block's sums of (Q, S): wave shuffles, then LDS; every thread gets them
__device__ __forceinline__ void temper_block_sum(unsigned long long &Q, unsigned long long &hi, unsigned long long &lo)
{
    __shared__ unsigned long long part[FILT_THREADS / WAVE][3];
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long ohi = __shfl_xor(hi, o), olo = __shfl_xor(lo, o);
        add_u128(hi, lo, ohi, olo);
        Q += __shfl_xor(Q, o);
    }
    if (threadIdx.x % WAVE == 0) {
        part[threadIdx.x / WAVE][0] = Q;
        part[threadIdx.x / WAVE][1] = lo;
        part[threadIdx.x / WAVE][2] = hi;
    }
    __syncthreads();
    Q = hi = lo = 0;
    for (int u = 0; u < FILT_THREADS / WAVE; u++) {
        Q += part[u][0];
        add_u128(hi, lo, part[u][2], part[u][1]);
    }
    __syncthreads();              // part may be reused by the next call
}

// One step of the procedure after trial `n_done` at k gave (Q, S): the trial recorded, {lo, hi} and the sums at lo
// updated.  Returns the next k, or the result with done set.
struct TemperSearch {
    long long k, lo, hi, done, trials, T;
    unsigned long long q_lo, s_lo_lo, s_lo_hi;         // Q_k and S_k at k = lo (k = 0: n 2^31, n 2^62)
};
__device__ __forceinline__ void temper_step(TemperSearch &t, unsigned long long Q, unsigned long long s_hi,
                                            unsigned long long s_lo, long long *trial_row)
{
    trial_row[0] = t.k;
    trial_row[1] = (long long)Q;
    trial_row[2] = (long long)s_lo;
    trial_row[3] = (long long)s_hi;
    const bool ok = temper_ok(Q, s_hi, s_lo, t.T);
    if (t.trials == 0 && ok) {
        t.lo = t.hi = TEMPER_STEPS;
        t.q_lo = Q, t.s_lo_lo = s_lo, t.s_lo_hi = s_hi;
    } else if (t.trials > 0 && ok) {
        t.lo = t.k;
        t.q_lo = Q, t.s_lo_lo = s_lo, t.s_lo_hi = s_hi;
    } else if (t.trials > 0) {
        t.hi = t.k;
    }                                                  // (trial 0 failed: lo = 0 and hi = 1024 as created)
    t.trials++;
    t.done = t.hi - t.lo > 1 ? 0 : 1;
    t.k = t.done ? t.lo : (t.lo + t.hi) >> 1;
}
__device__ __forceinline__ TemperSearch temper_begin(long long n, double floor_f)
{
    TemperSearch t;
    t.k = TEMPER_STEPS, t.lo = 0, t.hi = TEMPER_STEPS, t.done = 0, t.trials = 0;
    t.T = temper_target(floor_f, n);
    t.q_lo = (unsigned long long)n << 31;
    const unsigned __int128 s0 = (unsigned __int128)(unsigned long long)n << 62;
    t.s_lo_lo = (unsigned long long)s0, t.s_lo_hi = (unsigned long long)(s0 >> 64);
    return t;
}

// the table's row of a point: beta, the ESS at beta, T, the trials evaluated; not tempered (no counted member): NaN
__device__ __forceinline__ void temper_stats(const TemperSearch &t, bool tempered, double *st)
{
#pragma clang fp contract(off)
    if (!tempered) {
        for (int e = 0; e < TEMPER_WIDTH; e++) st[e] = __builtin_nan("");
        return;
    }
    st[0] = (double)t.k / (double)TEMPER_STEPS;
    st[1] = filter_ess(t.q_lo, t.s_lo_hi, t.s_lo_lo);
    st[2] = (double)t.T;
    st[3] = (double)t.trials;
}

// the draw of filter_draw on the tempered sum: the same Philox value x, qr[p] = {Q_k, floor(x Q_k / 2^64)}
__device__ __forceinline__ void temper_draw(unsigned long long seed, const long long *point_base, long long member_offset,
                                            long long p, long long members_per_point, unsigned row, unsigned long long Q,
                                            unsigned long long *qr)
{
    const unsigned long long key = point_base ? (unsigned long long)point_base[p]
                                              : (unsigned long long)(member_offset + p * members_per_point);
    const unsigned long long x = filter_philox64(seed, key, row);
    qr[2 * p] = Q;
    qr[2 * p + 1] = __umul64hi(x, Q);
}

// The bin path, one block per point after filter_weights_kernel: the row's bin counts n_b as that kernel forms them,
// d_b = l_b - s in LDS, and every trial inside the block -- the threads stride over the D bins with private sums, the
// block adds them, thread 0 compares and publishes the next k through LDS.  k < 1024: the point's bin table and draw are
// rewritten.  Every loop's trip count is block-uniform.
__global__ __launch_bounds__(FILT_THREADS) void filter_temper_bins_kernel(
    const unsigned short *w, long long members_per_point, int D, int obs, double dz, double sigma, double floor_f,
    unsigned long long seed, const long long *point_base, long long member_offset, unsigned row, long long n_arow,
    long long slot, long long *q_out, unsigned long long *qr, double *tstats, long long *trials)
{
#pragma clang fp contract(off)
    __shared__ unsigned bins[HC_MAX_DEPTH_NODES];
    __shared__ double dsh[HC_MAX_DEPTH_NODES];
    __shared__ long long ctl[2];                       // the next k, done
    for (int b = threadIdx.x; b < D; b += FILT_THREADS) bins[b] = 0;
    __syncthreads();
    const long long p = blockIdx.x;
    const long long m0 = p * members_per_point, m1 = m0 + members_per_point;
    const int lane = threadIdx.x % WAVE;
    for (long long k0 = m0 + (threadIdx.x - lane); k0 < m1; k0 += FILT_THREADS) {
        const long long k = k0 + lane;
        const int b = k < m1 ? (int)w[k] : -1;
        unsigned long long pending = __ballot(b >= 0 && b < D);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int v = __builtin_amdgcn_readlane(b, leader);
            const unsigned long long same = __ballot(b == v) & pending;
            if (lane == leader) atomicAdd(&bins[v], (unsigned)__popcll(same));
            pending &= ~same;
        }
    }
    __syncthreads();
    // l_b as filter_weights_kernel forms it; s = the largest over the occupied bins; n = the members counted
    double best = -INFINITY;
    unsigned long long n = 0, zero_hi = 0, zero_lo = 0;
    for (int b = threadIdx.x; b < D; b += FILT_THREADS) {
        const double t = dz * (double)(b - obs) / sigma;
        const double l = -0.5 * (t * t);
        dsh[b] = l;
        if (bins[b]) {
            best = l > best ? l : best;
            n += bins[b];
        }
    }
    const double s = filter_block_max(best);
    temper_block_sum(n, zero_hi, zero_lo);
    for (int b = threadIdx.x; b < D; b += FILT_THREADS) dsh[b] = dsh[b] - s;
    __syncthreads();
    long long *tr = trials + (size_t)p * TEMPER_TRIALS * TEMPER_WIDTH;
    double *st = tstats + ((size_t)p * n_arow + slot) * TEMPER_WIDTH;
    TemperSearch t = temper_begin((long long)n, floor_f);          // (thread 0's copy is the one that advances)
    if (n == 0) {
        if (threadIdx.x == 0) {
            for (int e = 0; e < TEMPER_TRIALS * TEMPER_WIDTH; e++) tr[e] = e % TEMPER_WIDTH == 0 ? -1 : 0;
            temper_stats(t, false, st);
        }
        return;
    }
    int k = TEMPER_STEPS;
    for (int trial = 0; trial < TEMPER_TRIALS; trial++) {
        unsigned long long Q = 0, hi = 0, lo = 0;
        for (int b = threadIdx.x; b < D; b += FILT_THREADS) {
            const unsigned long long nb = bins[b];
            if (nb) {
                const unsigned long long uq = (unsigned long long)temper_q(k, dsh[b]);
                Q += nb * uq;                                      // < 2^31 members x 2^31
                const unsigned long long sq = uq * uq;             // < 2^62
                add_u128(hi, lo, __umul64hi(sq, nb), sq * nb);
            }
        }
        temper_block_sum(Q, hi, lo);
        if (threadIdx.x == 0) {
            temper_step(t, Q, hi, lo, tr + trial * TEMPER_WIDTH);
            ctl[0] = t.k;
            ctl[1] = t.done;
        }
        __syncthreads();
        k = (int)ctl[0];
        const bool done = ctl[1] != 0;
        __syncthreads();
        if (done) break;
    }
    if (threadIdx.x == 0) {
        for (int e = (int)t.trials * TEMPER_WIDTH; e < TEMPER_TRIALS * TEMPER_WIDTH; e++) tr[e] = e % TEMPER_WIDTH == 0 ? -1 : 0;
        temper_stats(t, true, st);
        if (k < TEMPER_STEPS) temper_draw(seed, point_base, member_offset, p, members_per_point, row, t.q_lo, qr);
    }
    if (k < TEMPER_STEPS)
        for (int b = threadIdx.x; b < D; b += FILT_THREADS) q_out[(size_t)p * D + b] = bins[b] ? temper_q(k, dsh[b]) : 0;
}

// A sensor row, one trial's sums on the prefix scan's tiling: block (t, p) reads l_m and the index of its tile's
// members, takes the point's k from the search's state and writes the tile's {Q, S low, S high}.  A point that is done
// exits at once.
__global__ __launch_bounds__(FILT_THREADS) void filter_temper_sum_kernel(const unsigned short *w, long long members_per_point,
                                                                         int D, int width, long long n_tiles,
                                                                         const double *Y, const double *smax,
                                                                         const long long *state, unsigned long long *tpart)
{
#pragma clang fp contract(off)
    const long long p = blockIdx.y, t = blockIdx.x;
    const long long *st = state + (size_t)p * TEMPER_STATE;
    if (st[3]) return;
    const int k = (int)st[0];
    const double s = smax[p];
    unsigned long long Q = 0, hi = 0, lo = 0;
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = t * FILT_TILE + (long long)threadIdx.x * FILT_PER_THREAD + j;
        if (m >= members_per_point) continue;
        const size_t i = (size_t)(p * members_per_point + m);
        const double l = Y[i * width];
        if (!filter_counted((int)w[i], D, l)) continue;
        const unsigned long long uq = (unsigned long long)temper_q(k, l - s);
        Q += uq;
        add_u128(hi, lo, 0ull, uq * uq);
    }
    temper_block_sum(Q, hi, lo);
    if (threadIdx.x == 0) {
        unsigned long long *out = tpart + ((size_t)p * n_tiles + t) * 3;
        out[0] = Q;
        out[1] = lo;
        out[2] = hi;
    }
}

// ... and the decision, one block per point: the tiles' sums added (integers: no order), compared, {lo, hi} updated and
// the trial recorded.  first: trial 0 at k = 1024 on the sums filter_member_weights_kernel left (four words a tile, the
// last the members counted), which also creates the state and the hook's rows.
__global__ __launch_bounds__(FILT_THREADS) void filter_temper_decide_kernel(const unsigned long long *part, int stride,
                                                                            long long n_tiles, int first, double floor_f,
                                                                            long long *state, long long *trials)
{
    const long long p = blockIdx.x;
    long long *sw = state + (size_t)p * TEMPER_STATE;
    if (!first && sw[3]) return;
    unsigned long long Q = 0, hi = 0, lo = 0, n = 0, n_hi = 0, n_lo = 0;
    for (long long u = threadIdx.x; u < n_tiles; u += FILT_THREADS) {
        const unsigned long long *in = part + ((size_t)p * n_tiles + u) * stride;
        Q += in[0];
        add_u128(hi, lo, in[2], in[1]);
        if (first) n += in[3];
    }
    temper_block_sum(Q, hi, lo);
    if (first) temper_block_sum(n, n_hi, n_lo);
    if (threadIdx.x != 0) return;
    long long *tr = trials + (size_t)p * TEMPER_TRIALS * TEMPER_WIDTH;
    TemperSearch t;
    if (first) {
        for (int e = 0; e < TEMPER_TRIALS * TEMPER_WIDTH; e++) tr[e] = e % TEMPER_WIDTH == 0 ? -1 : 0;
        t = temper_begin((long long)n, floor_f);
        if (n == 0 || Q == 0) t.done = 2;
    } else {
        t.k = sw[0], t.lo = sw[1], t.hi = sw[2], t.done = sw[3], t.trials = sw[4], t.T = sw[5];
        t.q_lo = (unsigned long long)sw[6], t.s_lo_lo = (unsigned long long)sw[7], t.s_lo_hi = (unsigned long long)sw[8];
    }
    if (!t.done) temper_step(t, Q, hi, lo, tr + t.trials * TEMPER_WIDTH);
    sw[0] = t.k, sw[1] = t.lo, sw[2] = t.hi, sw[3] = t.done, sw[4] = t.trials, sw[5] = t.T;
    sw[6] = (long long)t.q_lo, sw[7] = (long long)t.s_lo_lo, sw[8] = (long long)t.s_lo_hi;
}

// ... and the result, on the tiling again: the table's row and, for a point with k < 1024, its members' q_m and its draw
// rewritten.  Y[m][m_s + 1] = exp(l_m - s) stays: W and the increment were formed from it.
__global__ __launch_bounds__(FILT_THREADS) void filter_temper_apply_kernel(
    const unsigned short *w, long long members_per_point, int D, int width, const double *Y, const double *smax,
    const long long *state, unsigned long long seed, const long long *point_base, long long member_offset, unsigned row,
    long long n_arow, long long slot, long long *qm, unsigned long long *qr, double *tstats)
{
#pragma clang fp contract(off)
    const long long p = blockIdx.y, t = blockIdx.x;
    const long long *sw = state + (size_t)p * TEMPER_STATE;
    const bool tempered = sw[3] == 1;
    const int k = (int)sw[0];
    if (t == 0 && threadIdx.x == 0) {
        TemperSearch ts;
        ts.k = sw[0], ts.lo = sw[1], ts.hi = sw[2], ts.done = sw[3], ts.trials = sw[4], ts.T = sw[5];
        ts.q_lo = (unsigned long long)sw[6], ts.s_lo_lo = (unsigned long long)sw[7], ts.s_lo_hi = (unsigned long long)sw[8];
        temper_stats(ts, tempered, tstats + ((size_t)p * n_arow + slot) * TEMPER_WIDTH);
        if (tempered && k < TEMPER_STEPS)
            temper_draw(seed, point_base, member_offset, p, members_per_point, row, ts.q_lo, qr);
    }
    if (!tempered || k >= TEMPER_STEPS) return;
    const double s = smax[p];
    for (int j = 0; j < FILT_PER_THREAD; j++) {
        const long long m = t * FILT_TILE + (long long)threadIdx.x * FILT_PER_THREAD + j;
        if (m >= members_per_point) continue;
        const size_t i = (size_t)(p * members_per_point + m);
        const double l = Y[i * width];
        qm[i] = filter_counted((int)w[i], D, l) ? temper_q(k, l - s) : 0;
    }
}

// ---- rejuvenation of the members' base noise vectors (hc_set_filter_rejuvenation, include/hydrocol.h)
// After a row's resampling, per point with 0 < survivors < N_p: the resampled vectors' mean and std per node by the
// EnKF's spread passes (enkf_spread_kernel + enkf_finish_kernel), Liu & West's shrinkage towards the mean plus a Philox
// jitter, then the spread passes again for the spread that is left.  Every decision is read on the device from the
// survivors count filter_fill_kernel left; contraction is off.
constexpr int REJUV_WIDTH = 4;                         // table entries per point and slot

__device__ __forceinline__ bool rejuv_applies(const unsigned long long *surv, long long p, long long mpp)
{
    const unsigned long long s = surv[p];
    return s > 0 && s < (unsigned long long)mpp;
}

// The two standard normals of the node pair q = d >> 1 under the filter's seed at counter (0x80000000 | q, row, gid_lo,
// gid_hi), with philox_normal's Box-Muller step: the cosine for the even node, the sine for the odd one.  A noise
// counter's first word is below 2^31, the perturbed forcing's are 0xFFFFFFE0 and 0xFFFFFFE1 and the filter's and the
// EnKF's are >= 0xFFFFFFF0: the streams never meet.
__device__ __forceinline__ void rejuv_normal_pair(unsigned long long seed, unsigned long long gid, unsigned row, uint32_t q,
                                                  double &even, double &odd)
{
#pragma clang fp contract(off)
    uint32_t r[4];
    philox4x32_10(0x80000000u | q, row, (uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const uint64_t a = ((uint64_t)r[1] << 32) | r[0], b = ((uint64_t)r[3] << 32) | r[2];
    const double u1 = ((double)(a >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(b >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    even = rad * c;
    odd = rad * s;
}

// the global member id of the handle's slot m: the id the EnKF's draws use
__device__ __forceinline__ unsigned long long rejuv_gid(const long long *point_base, long long member_offset, long long m,
                                                        long long mpp)
{
    return point_base ? (unsigned long long)(point_base[m / mpp] + m % mpp) : (unsigned long long)(member_offset + m);
}

// ---- perturbed forcing (hc_set_forcing_perturbation, include/hydrocol.h)
static_assert(FORCING_DAY_ROWS == HC_FORCING_DAY_ROWS, "one daily clock");
struct ForcingPert {
    double sigma[2], half[2];      // sigma_s and h_s = sigma_s^2 / 2
    double phi, c;
    unsigned long long seed;
};

// xi_{gid, day, s}: enkf_normal_at's block and Box-Muller step under the feature's seed at the stream's first word
__device__ __forceinline__ double forcing_normal(const ForcingPert &F, int s, unsigned long long gid, long long day)
{
    return enkf_normal_at(s ? HC_FORCING_WORD_DEMAND : HC_FORCING_WORD_PRECIP, F.seed, gid, (unsigned)day);
}

// Thread e = s * count + j: stream s of slot first + j.  It starts from the carried g (standing at day g_day >= 0) or,
// with none (g == NULL or g_day < 0), from g_0 = xi_0; walks the days up to day1 by the recursion; stores the factor of
// every day >= day0 into fmul [day1 - day0 + 1][2][count] (consecutive threads, consecutive addresses) and, where g_out
// is given, g of day1 into it: the host's second buffer, which replaces the carried one once the step launch is issued.
// The host guarantees g_day <= day0 <= day1.
__global__ __launch_bounds__(256) void forcing_factor_fill_kernel(const double *g, double *g_out, long long g_day,
                                                                  long long g_stride, double *fmul,
                                                                  long long first, long long count, long long day0,
                                                                  long long day1, long long mpp, const long long *point_base,
                                                                  long long member_offset, const ForcingPert F)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * count) return;
    const int s = (int)(e / count);
    const long long j = e % count, m = first + j;
    const unsigned long long gid = rejuv_gid(point_base, member_offset, m, mpp);
    const bool carried = g != nullptr && g_day >= 0;
    long long d = carried ? g_day : 0;
    double gv = carried ? g[(size_t)s * g_stride + m] : forcing_normal(F, s, gid, 0);
    for (;;) {
        if (d >= day0) {
            const double sg = F.sigma[s] * gv;
            fmul[(size_t)((d - day0) * 2 + s) * count + j] = F.sigma[s] == 0.0 ? 1.0 : exp(sg - F.half[s]);
        }
        if (d >= day1) break;
        d++;
        const double keep = F.phi * gv, fresh = F.c * forcing_normal(F, s, gid, d);
        gv = keep + fresh;
    }
    if (g_out) g_out[(size_t)s * g_stride + m] = gv;
}

// the raw normals of one stream key: out[n_days][2] (hc_forcing_normals)
__global__ void forcing_normals_kernel(double *out, unsigned long long gid, long long first_day, long long n_days,
                                       const ForcingPert F)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * n_days) return;
    out[e] = forcing_normal(F, (int)(e % 2), gid, first_day + e / 2);
}

// One wave per member, the column layout of enkf_relax_kernel (node c * WAVE + lane in slot c):
// z'_d = mean_d + a (z_d - mean_d) + (h s_d) eps_d from mom = (mean, s) [P][3][D], stored only when every entry is
// finite (enkf_keep_column's vote; else the member keeps its vector and is counted in refused[p]).  Lane l forms the
// normals of the pairs c2 * WAVE + l -- one Philox block, one log and one sincospi for both nodes -- and a shuffle brings
// node d's to the lane that holds it: nodes (2 c2 + j) WAVE + lane, j = 0, 1, are pair c2 WAVE + 32 j + lane / 2.
__global__ __launch_bounds__(256) void filter_rejuvenate_kernel(double *base, const double *mom,
                                                                const unsigned long long *surv, long long n_members,
                                                                long long mpp, int D, double a, double hh,
                                                                unsigned long long seed, const long long *point_base,
                                                                long long member_offset, unsigned row,
                                                                unsigned long long *refused)
{
#pragma clang fp contract(off)
    static_assert(ENKF_SLOTS % 2 == 0, "the pairs of a wave cover two slots");
    const int lane = threadIdx.x % WAVE;
    const long long waves = (long long)gridDim.x * (blockDim.x / WAVE);
    for (long long m = (long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE; m < n_members; m += waves) {
        const long long p = m / mpp;
        if (!rejuv_applies(surv, p, mpp)) continue;                   // (wave-uniform)
        const unsigned long long gid = rejuv_gid(point_base, member_offset, m, mpp);
        const double *mean = mom + (size_t)p * 3 * D, *sd = mean + D;
        double *col = base + (size_t)m * D;
        double z[ENKF_SLOTS], next[ENKF_SLOTS];
#pragma unroll
        for (int c2 = 0; c2 < ENKF_SLOTS / 2; c2++) {
            const int q = c2 * WAVE + lane;
            double even = 0.0, odd = 0.0;
            if (2 * q < D) rejuv_normal_pair(seed, gid, row, (uint32_t)q, even, odd);
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int c = 2 * c2 + j, d = c * WAVE + lane, src = (WAVE / 2) * j + lane / 2;
                const double ve = __shfl(even, src), vo = __shfl(odd, src);
                const double eps = lane & 1 ? vo : ve;
                z[c] = 0.0;
                next[c] = 0.0;
                if (d < D) {
                    const double mu = mean[d];
                    z[c] = col[d];
                    next[c] = (mu + a * (z[c] - mu)) + (hh * sd[d]) * eps;
                }
            }
        }
        const bool keep = enkf_keep_column(z, next, col, lane, D);
        if (!keep && lane == 0) atomicAdd(refused + p, 1ull);
    }
}

// The moments and the table's row from the sums of two spread passes over the base vectors (s1: of x - x_0; s2: of the
// squared anomalies), one block per point, thread d = node d.  after = 0, the resampled vectors: mom[p][0] = mean_d =
// x_0d + s1_d / N_p and mom[p][1] = s_d = sqrt(s2_d / (N_p - 1)) (N_p = 1: 0), entries 0 and 2 of the row, 1 and 3
// created.  after = 1, the vectors the move left: mom[p][2] = s_d, entries 1 (the members refused) and 3.  Entries 2
// and 3, sqrt(sum_d s_d^2 / D), are summed by thread 0, nodes ascending; NaN where the point was not rejuvenated.
__global__ __launch_bounds__(HC_MAX_DEPTH_NODES) void filter_rejuv_diag_kernel(
    const double *base, const double *s1, const double *s2, const unsigned long long *surv, const unsigned long long *refused,
    long long mpp, int D, int after, double *mom, double *table, long long n_arow, long long slot)
{
#pragma clang fp contract(off)
    __shared__ double sq[HC_MAX_DEPTH_NODES];
    const long long p = blockIdx.x;
    const int d = threadIdx.x;
    if (d < D) {
        const size_t k = (size_t)p * D + d;
        const double s = mpp > 1 ? sqrt(s2[k] / (double)(mpp - 1)) : 0.0;
        double *mo = mom + (size_t)p * 3 * D;
        if (!after) {
            mo[d] = base[(size_t)(p * mpp) * D + d] + s1[k] / (double)mpp;
            mo[D + d] = s;
        } else {
            mo[2 * D + d] = s;
        }
        sq[d] = s * s;
    }
    __syncthreads();
    if (d != 0) return;
    const bool applied = rejuv_applies(surv, p, mpp);
    double sum = 0.0;
    for (int i = 0; i < D; i++) sum += sq[i];
    const double spread = applied ? sqrt(sum / (double)D) : __builtin_nan("");
    double *st = table + ((size_t)p * n_arow + slot) * REJUV_WIDTH;
    if (!after) {
        st[0] = applied ? 1.0 : 0.0;
        st[1] = 0.0;
        st[2] = spread;
        st[3] = __builtin_nan("");
    } else {
        st[1] = (double)refused[p];
        st[3] = spread;
    }
}

// the normals of slots first ... first + count - 1 at `row` as filter_rejuvenate_kernel forms them, out [count][D]; one
// thread per slot and node pair (hc_filter_rejuvenation_normals)
__global__ void filter_rejuv_normals_kernel(unsigned long long seed, const long long *point_base, long long member_offset,
                                            long long mpp, unsigned row, long long first, long long count, int D, double *out)
{
    const int pairs = (D + 1) / 2;
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count * pairs) return;
    const long long j = k / pairs;
    const int q = (int)(k % pairs);
    double even, odd;
    rejuv_normal_pair(seed, rejuv_gid(point_base, member_offset, first + j, mpp), row, (uint32_t)q, even, odd);
    out[(size_t)j * D + 2 * q] = even;
    if (2 * q + 1 < D) out[(size_t)j * D + 2 * q + 1] = odd;
}

__global__ void widen_u16(const unsigned short *in, int *out, size_t n)
{
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = in[k];
}

// T_RDELTA of every point: the refined reciprocal of por - theta_res, by the cell model's own instruction sequence
__global__ void fill_rdelta(double *tab, const ColumnDev *P, int slots)
{
    double *t = tab + (size_t)blockIdx.x * NTAB * slots;
    const double theta_res = P[blockIdx.x].theta_res;
    for (int k = threadIdx.x; k < slots; k += blockDim.x)
        t[(size_t)T_RDELTA * slots + k] = refined_rcp(t[(size_t)T_POR * slots + k] - theta_res);
}
__global__ void fill_d(double *p, double v, size_t n)
{
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) p[k] = v;
}

// src holds one column per parameter point ([n_points][D]; one point: a single column for everybody)
__global__ void broadcast_state(const double *src, double *dst, int D, long long n_members, long long members_per_point)
{
    size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < (size_t)D * n_members) dst[k] = src[((k / D) / members_per_point) * D + k % D];
}

__global__ void philox_dump(unsigned long long seed, long long member, unsigned draw, int D, double *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < D) out[i] = philox_normal(seed, (unsigned long long)member, draw, (unsigned)i);
}

// plugin call on the nodes (diagnostics), one thread per (member, node)
__global__ void model_nodes_kernel(const StepArgs A, const double *node_tabs, int special, double *out,
                                   double *qinf)
{
    const IoArgs io = load_const(A.io);
    const int D = A.D;
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)A.n_members * D;
    if (k >= total) return;
    const long long member = k / D;
    const int i = (int)(k % D);
    const long long point = member / A.members_per_point;
    const ColumnDev P = A.P[point];
    node_tabs += (size_t)point * 3 * D;
    const double por = node_tabs[i], meank = node_tabs[D + i], noisec = node_tabs[2 * D + i];
    const double mk = meank == 0.0 ? 1.0e-7 : meank;
    double z;
    if (A.host_noise)
        z = io.base_noise[member * D + i];
    else
    {
        const long long gid = A.n_points > 1 ? io.point_base[point] + (member - point * A.members_per_point)
                                             : io.member_offset + member;
        z = philox_normal(io.seed, (unsigned long long)gid, 0u, (unsigned)i) * io.nscale[member];
    }
    double th, K, C, kb, pf;
    if (special)
        model_cell<true>(P, io.psi[k], por, 1.0 / (por - P.theta_res), log(mk), 1.0 / (mk * mk), noisec, noisec * z, th, K, C, kb, pf);
    else
        model_cell<false>(P, io.psi[k], por, 1.0 / (por - P.theta_res), log(mk), 1.0 / (mk * mk), noisec, noisec * z, th, K, C, kb, pf);
    out[k] = th;
    out[total + k] = K;
    out[2 * total + k] = C;
    out[3 * total + k] = kb;
    if (qinf && i == 0) qinf[member] = fmin(2.0 * (por - th) * P.dz, kb);
}

// Stateless plugin call on arbitrary depths: psi [n_cells][n_cols] (depth-major, the reference's [dim_d x dim_m]),
// per-cell tables and noise [n_cells]; out [4][n_cells][n_cols] = theta, K, C, K_bkg; qinf [n_cols] from row 0
// (vrettas_fung.py:51-257, vanGenuchten.py:23-126).
__global__ void plugin_kernel(const ColumnDev P, int special, long long n_cells, long long n_cols, const double *psi,
                              const double *por, const double *meank, const double *noisec, const double *n_rnd,
                              double *out, double *qinf)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)n_cells * n_cols;
    if (k >= total) return;
    const long long i = k / n_cols;
    const double mk = meank[i] == 0.0 ? 1.0e-7 : meank[i];
    double th, K, C, kb, pf;
    if (special)
        model_cell<true>(P, psi[k], por[i], 0.0, log(mk), 1.0 / (mk * mk), noisec[i], noisec[i] * n_rnd[i], th, K, C, kb, pf);
    else
        model_cell<false>(P, psi[k], por[i], 0.0, log(mk), 1.0 / (mk * mk), noisec[i], noisec[i] * n_rnd[i], th, K, C, kb, pf);
    out[k] = th;
    out[total + k] = K;
    out[2 * total + k] = C;
    out[3 * total + k] = kb;
    if (i == 0) qinf[k] = fmin(2.0 * (por[0] - th) * P.dz, kb);
}

}  // namespace hc

// ------------------------------------------------------------------ launch dispatch
namespace {

// kernel launch through the per-CPL translation units (hc_launch.h).  HC_CPL_MASK (bit n = cells-per-lane count n is
// linked in) lets development builds carry a few depths only.
#ifndef HC_CPL_MASK
#define HC_CPL_MASK 0x7FC
#endif
hipError_t launch_step_cpl_any(int cpl, bool &known, const LaunchCfg &cfg, const StepArgs &A)
{
    known = true;
    switch (cpl) {
#if (HC_CPL_MASK >> 2) & 1
        case 2: return launch_step_cpl<2>(cfg, A);
#endif
#if (HC_CPL_MASK >> 3) & 1
        case 3: return launch_step_cpl<3>(cfg, A);
#endif
#if (HC_CPL_MASK >> 4) & 1
        case 4: return launch_step_cpl<4>(cfg, A);
#endif
#if (HC_CPL_MASK >> 5) & 1
        case 5: return launch_step_cpl<5>(cfg, A);
#endif
#if (HC_CPL_MASK >> 6) & 1
        case 6: return launch_step_cpl<6>(cfg, A);
#endif
#if (HC_CPL_MASK >> 7) & 1
        case 7: return launch_step_cpl<7>(cfg, A);
#endif
#if (HC_CPL_MASK >> 8) & 1
        case 8: return launch_step_cpl<8>(cfg, A);
#endif
#if (HC_CPL_MASK >> 9) & 1
        case 9: return launch_step_cpl<9>(cfg, A);
#endif
#if (HC_CPL_MASK >> 10) & 1
        case 10: return launch_step_cpl<10>(cfg, A);
#endif
        default: break;
    }
    known = false;
    return hipSuccess;
}
hipError_t launch_rhs_cpl_any(int cpl, bool &known, const LaunchCfg &cfg, const StepArgs &A, long long row, double *dydt, double *aux, double *diag)
{
    known = true;
    switch (cpl) {
#if (HC_CPL_MASK >> 2) & 1
        case 2: return launch_rhs_cpl<2>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 3) & 1
        case 3: return launch_rhs_cpl<3>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 4) & 1
        case 4: return launch_rhs_cpl<4>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 5) & 1
        case 5: return launch_rhs_cpl<5>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 6) & 1
        case 6: return launch_rhs_cpl<6>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 7) & 1
        case 7: return launch_rhs_cpl<7>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 8) & 1
        case 8: return launch_rhs_cpl<8>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 9) & 1
        case 9: return launch_rhs_cpl<9>(cfg, A, row, dydt, aux, diag);
#endif
#if (HC_CPL_MASK >> 10) & 1
        case 10: return launch_rhs_cpl<10>(cfg, A, row, dydt, aux, diag);
#endif
        default: break;
    }
    known = false;
    return hipSuccess;
}

int unknown_depth(hc_handle *h)
{
    return fail(HC_ERR_UNSUPPORTED, "D = %d needs %d cells per lane; this build covers D <= %d (depth mask 0x%x)",
                h->p.dim_d, h->cpl, HC_MAX_DEPTH_NODES, HC_CPL_MASK);
}

LaunchCfg launch_cfg(hc_handle *h, unsigned grid, bool step = false)
{
    // PREDICT is per point in the tables but one kernel serves the launch: any predictive point selects the build
    // with the branch compiled in; a monitoring-mode point inside such a launch keeps its own semantics (flag_predict).
    // Those builds also carry the perturbed forcing's two products, so a step launch with the feature on takes them
    // (the RHS hooks stay with the record and with the build they had).
    bool predict = step && h->fp_on;
    for (const ColumnDev &P : h->P_host) predict = predict || P.flag_predict;
    return LaunchCfg{h->stream, grid, h->use_special(), predict};
}

int launch_step(hc_handle *h, const StepArgs &A)
{
    const int wpb = wpb_of(h->cpl, 1, h->use_special());
    HIP_TRY(hipMemsetAsync(h->counters.p + 63, 0, sizeof(unsigned long long), h->stream));
    if (h->use_pair()) {
        // split column: a workgroup runs two members at a time, two waves each
        const int pairs = wpb_of(PAIR_CPL, 2) / 2;
        const long long want = (A.n_members + pairs - 1) / pairs;
        const unsigned grid = (unsigned)std::min<long long>(want, (long long)h->n_cu);
        StepArgs B = A;
        B.tab = h->tab_pair.p;
        B.gtab = h->gtab_pair.p;
        HIP_TRY(launch_step_pair(launch_cfg(h, grid, true), B));
        return HC_OK;
    }
    // persistent grid: LDS admits one workgroup per CU; fewer workgroups when there are fewer members
    const long long want = (A.n_members + wpb - 1) / wpb;
    const unsigned grid = (unsigned)std::min<long long>(want, (long long)h->n_cu);
    bool known = false;
    const hipError_t err = launch_step_cpl_any(h->cpl, known, launch_cfg(h, grid, true), A);
    if (!known) return unknown_depth(h);
    HIP_TRY(err);
    return HC_OK;
}

// variant (include/hydrocol.h, hc_rhs_ex): HC_RHS_HOOK keeps a split column's c | s | f view on the one-wave hook, as
// hc_rhs always has; the other two follow the step kernel's routing, with the step kernel's rhs_eval (HC_RHS_AS_STEPPED)
// or the plain one (HC_RHS_HOOK_LAYOUT)
int launch_rhs(hc_handle *h, const StepArgs &A, long long row, int variant, double *dydt, double *aux, double *diag)
{
    const int wpb = wpb_of(h->cpl, 1, h->use_special());
    if (h->use_pair() && (!aux || variant != HC_RHS_HOOK)) {          // the split-column code path
        StepArgs B = A;
        B.tab = h->tab_pair.p;
        B.gtab = h->gtab_pair.p;
        const int pairs = wpb_of(PAIR_CPL, 2) / 2;
        LaunchCfg cfg = launch_cfg(h, (unsigned)((A.n_members + pairs - 1) / pairs));
        cfg.as_stepped = variant == HC_RHS_AS_STEPPED;
        HIP_TRY(launch_rhs_pair(cfg, B, row, dydt, aux, diag));
        return HC_OK;
    }
    LaunchCfg cfg = launch_cfg(h, (unsigned)((A.n_members + wpb - 1) / wpb));
    cfg.as_stepped = variant == HC_RHS_AS_STEPPED;
    bool known = false;
    const hipError_t err = launch_rhs_cpl_any(h->cpl, known, cfg, A, row, dydt, aux, diag);
    if (!known) return unknown_depth(h);
    HIP_TRY(err);
    return HC_OK;
}

// ------------------------------------------------------------------ accumulated tables (AccTable)
// Each `ensure_*` applies the table's own rules, then has the table exist, zeroed, for the current shape key.
// the moment tables exist once forcing and column are known: [n_points][3][n_rows]; hc_set_forcing resets them
int ensure_moments(hc_handle *h)
{
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    return h->moments.ensure(h->n_points, 0, 0, (int64_t)h->n_points * 3 * h->n_rows);
}

// Word offsets of the profile-statistics table (include/hydrocol.h, hc_set_profile_stats)
struct ProfLayout {
    int64_t n_prow = 0, prof = 0, pcnt = 0, flux = 0, fcnt = 0, aerr = 0, ovf = 0, words = 0;
};
ProfLayout prof_layout(const hc_handle *h)
{
    ProfLayout L;
    const int64_t P = h->n_points, T = h->n_rows, D = h->p.dim_d;
    L.n_prow = (T - 1) / h->prof_stride + 1;
    L.pcnt = L.prof + P * L.n_prow * D * 2 * HC_PROF_WORDS;
    L.flux = L.pcnt + P * L.n_prow;
    L.fcnt = L.flux + P * T * 2 * HC_PROF_WORDS;
    L.aerr = L.fcnt + P * T;
    L.ovf = L.aerr + P * T;
    L.words = L.ovf + 1;
    return L;
}
int ensure_prof(hc_handle *h)
{
    if (h->prof_stride <= 0) return fail(HC_ERR_ARG, "profile statistics are off (hc_set_profile_stats)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    return h->prof.ensure(h->n_points, h->n_rows, h->p.dim_d, prof_layout(h).words);
}

// the water-table histogram table (hc_set_wtd_hist): [P][hist_rows][D] int32
int64_t hist_rows(const hc_handle *h) { return (h->n_rows - 1) / h->hist_stride + 1; }
int64_t hist_entries(const hc_handle *h) { return (int64_t)h->n_points * hist_rows(h) * h->p.dim_d; }
int ensure_hist(hc_handle *h)
{
    if (h->hist_stride <= 0) return fail(HC_ERR_ARG, "water-table histograms are off (hc_set_wtd_hist)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    if (h->n_members / std::max(h->n_points, 1) > INT32_MAX)
        return fail(HC_ERR_ARG, "water-table histograms: %lld members per point do not fit an int32 bin",
                    (long long)(h->n_members / std::max(h->n_points, 1)));
    if (hist_entries(h) > HC_WTD_HIST_MAX_ENTRIES)
        return fail(HC_ERR_ARG, "water-table histograms: %lld entries exceed HC_WTD_HIST_MAX_ENTRIES (take a longer stride)",
                    (long long)hist_entries(h));
    return h->hist.ensure(h->n_points, h->n_rows, h->p.dim_d, hist_entries(h));
}

// the soil-moisture histogram table (hc_set_theta_hist): [P][n_prow][D][B] int32 on the profile rows, then the outside
// count (one uint64 in two entries; the bins before it are a multiple of 32 entries, so it is 8-byte aligned)
int64_t thist_bins_total(const hc_handle *h)
{
    return (int64_t)h->n_points * prof_layout(h).n_prow * h->p.dim_d * h->thist_bins;
}
int ensure_thist(hc_handle *h)
{
    if (h->thist_bins <= 0) return fail(HC_ERR_ARG, "soil-moisture histograms are off (hc_set_theta_hist)");
    if (h->prof_stride <= 0)
        return fail(HC_ERR_ARG, "soil-moisture histograms need the profile statistics (hc_set_profile_stats)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    if (h->n_members / std::max(h->n_points, 1) > INT32_MAX)
        return fail(HC_ERR_ARG, "soil-moisture histograms: %lld members per point do not fit an int32 bin",
                    (long long)(h->n_members / std::max(h->n_points, 1)));
    if (thist_bins_total(h) > HC_WTD_HIST_MAX_ENTRIES)
        return fail(HC_ERR_ARG, "soil-moisture histograms: %lld entries exceed HC_WTD_HIST_MAX_ENTRIES (take a longer "
                    "profile stride or fewer bins)", (long long)thist_bins_total(h));
    return h->thist.ensure(h->n_points, h->n_rows, h->p.dim_d, thist_bins_total(h) + 2);
}

// the theta covariance table (hc_set_theta_cov): int64 [P][n_prow][W] on the profile rows, then the outside word
struct CovLayout {
    int s = 0, n = 0, E = 0, E64 = 0;
    int64_t W = 0, words = 0;
};
CovLayout cov_layout(const hc_handle *h)
{
    CovLayout C;
    C.s = h->cov_stride;
    C.n = (h->p.dim_d + C.s - 1) / C.s;
    C.E = C.n + 1;
    C.E64 = (C.E + COV_TILE - 1) / COV_TILE * COV_TILE;
    C.W = 1 + C.E + (int64_t)C.E * (C.E + 1) / 2;
    C.words = (int64_t)h->n_points * prof_layout(h).n_prow * C.W + 1;
    return C;
}
int ensure_cov(hc_handle *h)
{
    if (h->cov_stride <= 0) return fail(HC_ERR_ARG, "the theta covariance is off (hc_set_theta_cov)");
    if (h->prof_stride <= 0)
        return fail(HC_ERR_ARG, "the theta covariance needs the profile statistics (hc_set_profile_stats)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    if (h->cov_stride > h->p.dim_d)
        return fail(HC_ERR_ARG, "theta covariance: node stride %d exceeds the column's %d nodes", h->cov_stride,
                    (int)h->p.dim_d);
    if (h->n_members / std::max(h->n_points, 1) > HC_THETA_COV_MAX_MEMBERS)
        return fail(HC_ERR_ARG, "theta covariance: %lld members per point exceed HC_THETA_COV_MAX_MEMBERS (2^22: the sums "
                    "of products stay within 2^62)", (long long)(h->n_members / std::max(h->n_points, 1)));
    const CovLayout C = cov_layout(h);
    if (C.words - 1 > HC_THETA_COV_MAX_WORDS)
        return fail(HC_ERR_ARG, "theta covariance: %lld words exceed HC_THETA_COV_MAX_WORDS (take a larger node stride or a "
                    "larger profile stride)", (long long)(C.words - 1));
    return h->cov.ensure(h->n_points, h->n_rows, h->p.dim_d, C.words);
}

// the layer-storage tables (hc_set_layer_storage): int64 stor [P][n_prow][L][5], scnt [P][n_prow], ovf [1]; with bins the
// int32 hist [P][n_prow][L][B] and the outside count (one uint64 in two entries, 8-byte aligned behind a multiple of 32)
struct StorLayout {
    int64_t scnt = 0, ovf = 0, words = 0, bins = 0;
};
StorLayout stor_layout(const hc_handle *h)
{
    StorLayout S;
    const int64_t slots = (int64_t)h->n_points * prof_layout(h).n_prow;
    S.scnt = slots * h->stor_layers * HC_PROF_WORDS;
    S.ovf = S.scnt + slots;
    S.words = S.ovf + 1;
    S.bins = slots * h->stor_layers * h->stor_bins;
    return S;
}
int ensure_stor(hc_handle *h)
{
    if (h->stor_layers <= 0) return fail(HC_ERR_ARG, "layer storage is off (hc_set_layer_storage)");
    if (h->prof_stride <= 0) return fail(HC_ERR_ARG, "layer storage needs the profile statistics (hc_set_profile_stats)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    for (int l = 0; l < h->stor_layers; l++) {
        const int i0 = h->stor_range[l][0], i1 = h->stor_range[l][1];
        if (i0 < 0 || i0 >= i1 || i1 > h->p.dim_d)
            return fail(HC_ERR_ARG, "layer storage: layer %d is [%d, %d), not a range of nodes 0 <= i0 < i1 <= %d", l, i0, i1,
                        (int)h->p.dim_d);
        if ((double)(i1 - i0) * h->p.dz >= HC_STORAGE_MAX_CM)
            return fail(HC_ERR_ARG, "layer storage: layer %d is %g cm thick (less than %g cm fit the moments)", l,
                        (double)(i1 - i0) * h->p.dz, HC_STORAGE_MAX_CM);
    }
    if (h->n_members / std::max(h->n_points, 1) > INT32_MAX)
        return fail(HC_ERR_ARG, "layer storage: %lld members per point do not fit an int32 bin",
                    (long long)(h->n_members / std::max(h->n_points, 1)));
    const StorLayout S = stor_layout(h);
    if (S.bins > HC_WTD_HIST_MAX_ENTRIES)
        return fail(HC_ERR_ARG, "layer storage: %lld histogram entries exceed HC_WTD_HIST_MAX_ENTRIES", (long long)S.bins);
    if (int rc = h->stor.ensure(h->n_points, h->n_rows, h->p.dim_d, S.words)) return rc;
    return h->stor_bins > 0 ? h->shist.ensure(h->n_points, h->n_rows, h->p.dim_d, S.bins + 2) : HC_OK;
}
int ensure_stor_hist(hc_handle *h)
{
    if (int rc = ensure_stor(h)) return rc;
    return h->stor_bins > 0 ? HC_OK : fail(HC_ERR_ARG, "layer storage has no histogram (hc_set_layer_storage with n_bins = 0)");
}

// the conductivity table (hc_set_conductivity_stats): int64 kmom [P][n_prow][D][2][5], kcnt [P][n_prow][D][2], kmom_layer
// [P][n_prow][L][5], kcnt_layer [P][n_prow][L], ovf [1]
struct CondLayout {
    int64_t kcnt = 0, kmom_layer = 0, kcnt_layer = 0, ovf = 0, words = 0;
};
CondLayout cond_layout(const hc_handle *h)
{
    CondLayout C;
    const int64_t slots = (int64_t)h->n_points * prof_layout(h).n_prow, D = h->p.dim_d, L = h->cond_layers;
    C.kcnt = slots * D * 2 * HC_PROF_WORDS;
    C.kmom_layer = C.kcnt + slots * D * 2;
    C.kcnt_layer = C.kmom_layer + slots * L * HC_PROF_WORDS;
    C.ovf = C.kcnt_layer + slots * L;
    C.words = C.ovf + 1;
    return C;
}
void cond_off(hc_handle *h)
{
    h->cond_on = false;
    h->cond_layers = 0;
    h->cond.release();
}
int ensure_cond(hc_handle *h)
{
    if (!h->cond_on) return fail(HC_ERR_ARG, "the conductivity statistics are off (hc_set_conductivity_stats)");
    if (h->prof_stride <= 0)
        return fail(HC_ERR_ARG, "the conductivity statistics need the profile statistics (hc_set_profile_stats)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    for (int l = 0; l < h->cond_layers; l++) {
        const int i0 = h->cond_range[l][0], i1 = h->cond_range[l][1];
        if (i0 < 0 || i0 >= i1 || i1 > h->p.dim_d)
            return fail(HC_ERR_ARG, "conductivity statistics: layer %d is [%d, %d), not a range of nodes 0 <= i0 < i1 <= %d", l,
                        i0, i1, (int)h->p.dim_d);
        if ((double)(i1 - i0) * h->p.dz >= HC_STORAGE_MAX_CM)
            return fail(HC_ERR_ARG, "conductivity statistics: layer %d is %g cm thick (less than %g cm, the layer storage's rule)",
                        l, (double)(i1 - i0) * h->p.dz, HC_STORAGE_MAX_CM);
    }
    return h->cond.ensure(h->n_points, h->n_rows, h->p.dim_d, cond_layout(h).words);
}

// the period-totals tables (hc_set_period_totals): int64 pmom [P][n_period][K][5], pcnt [P][n_period], ovf [1]; with bins
// the int32 phist_flux [P][n_period][2][B], phist_wtd [P][n_period][2][D] and the outside count (one uint64 in two
// entries, 8-byte aligned behind an even count)
struct PeriodLayout {
    int K = 0;
    int64_t pcnt = 0, ovf = 0, words = 0, wtd = 0, entries = 0;
};
PeriodLayout period_layout(const hc_handle *h)
{
    PeriodLayout L;
    const int64_t slots = (int64_t)h->n_points * h->per_n;
    L.K = 4 + h->per_nthr;
    L.pcnt = slots * L.K * HC_PROF_WORDS;
    L.ovf = L.pcnt + slots;
    L.words = L.ovf + 1;
    L.wtd = slots * 2 * h->per_bins;
    L.entries = h->per_bins > 0 ? slots * 2 * ((int64_t)h->per_bins + h->p.dim_d) : 0;
    return L;
}
int ensure_period(hc_handle *h)
{
    if (h->per_n <= 0) return fail(HC_ERR_ARG, "period totals are off (hc_set_period_totals)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    if (h->per_end.back() >= h->n_rows)
        return fail(HC_ERR_ARG, "period totals: the last end row %lld is not below the %lld forcing rows",
                    (long long)h->per_end.back(), (long long)h->n_rows);
    for (int j = 0; j < h->per_nthr; j++)
        if (h->per_thr[j] < 0 || h->per_thr[j] >= h->p.dim_d)
            return fail(HC_ERR_ARG, "period totals: threshold node %d is outside the column's %d nodes", h->per_thr[j],
                        (int)h->p.dim_d);
    if (h->fs_n > 0)
        return fail(HC_ERR_ARG, "period totals with a sharded particle filter (hc_set_filter_shard): the routed columns do "
                                "not carry the members' accumulators");
    if (h->n_members / std::max(h->n_points, 1) > INT32_MAX)
        return fail(HC_ERR_ARG, "period totals: %lld members per point do not fit an int32 bin",
                    (long long)(h->n_members / std::max(h->n_points, 1)));
    const PeriodLayout L = period_layout(h);
    if (L.entries > HC_WTD_HIST_MAX_ENTRIES)
        return fail(HC_ERR_ARG, "period totals: %lld histogram entries exceed HC_WTD_HIST_MAX_ENTRIES", (long long)L.entries);
    if (int rc = h->pmom.ensure(h->n_points, h->n_rows, h->p.dim_d, L.words)) return rc;
    if (h->per_bins > 0)
        if (int rc = h->phist.ensure(h->n_points, h->n_rows, h->p.dim_d, L.entries + 2)) return rc;
    const int64_t N = h->n_members;
    if (N > 0 && !(h->pacc.key[0] == N && h->pacc.key[1] == L.K && h->pacc.key[2] == 0)) {
        // fresh accumulators: sums and counts 0, the minimum 65535, the maximum 0
        if (int rc = h->pacc.ensure(N, L.K, 0, N * L.K)) return rc;
        const std::vector<long long> none((size_t)N, PERIOD_WTD_NONE);
        HIP_TRY(hipMemcpy(h->pacc.buf.p + 2 * N, none.data(), (size_t)N * 8, hipMemcpyHostToDevice));
    }
    return HC_OK;
}
int ensure_period_hist(hc_handle *h)
{
    if (int rc = ensure_period(h)) return rc;
    return h->per_bins > 0 ? HC_OK : fail(HC_ERR_ARG, "period totals have no histograms (hc_set_period_totals with n_bins = 0)");
}
int ensure_period_acc(hc_handle *h)
{
    if (int rc = ensure_period(h)) return rc;
    return h->n_members > 0 ? HC_OK : fail(HC_ERR_ARG, "period totals: no members yet (hc_set_members / hc_set_state)");
}

// the root-uptake tables (hc_set_root_uptake): int64 umom [P][n_period][L + 1][5], ucnt [P][n_period], uprof
// [P][n_period][D - 1][2], ovf [1]; with bins the int32 share histograms [P][n_period][L][B] and the outside count (one
// uint64 in two entries, 8-byte aligned behind a multiple of 32)
struct UptLayout {
    int K = 0;
    int64_t ucnt = 0, uprof = 0, ovf = 0, words = 0, bins = 0;
};
UptLayout uptake_layout(const hc_handle *h)
{
    UptLayout U;
    const int64_t slots = (int64_t)h->n_points * h->per_n;
    U.K = h->upt_layers + 1;
    U.ucnt = slots * U.K * HC_PROF_WORDS;
    U.uprof = U.ucnt + slots;
    U.ovf = U.uprof + slots * (h->p.dim_d - 1) * 2;
    U.words = U.ovf + 1;
    U.bins = slots * h->upt_layers * h->upt_bins;
    return U;
}
void uptake_off(hc_handle *h)
{
    h->upt_layers = h->upt_bins = 0;
    h->uacc.release(), h->uacc_alt.release(), h->upt.release(), h->uhist.release(), h->mid_tabs.release();
    h->mid_dirty = true;
}
int ensure_uptake(hc_handle *h)
{
    if (h->upt_layers <= 0) return fail(HC_ERR_ARG, "root uptake is off (hc_set_root_uptake)");
    if (h->per_n <= 0) return fail(HC_ERR_ARG, "root uptake needs the period totals (hc_set_period_totals)");
    if (int rc = ensure_period(h)) return rc;
    const int M = h->p.dim_d - 1;
    for (int l = 0; l < h->upt_layers; l++) {
        const int c0 = h->upt_range[l][0], c1 = h->upt_range[l][1];
        if (c0 < 0 || c0 >= c1 || c1 > M)
            return fail(HC_ERR_ARG, "root uptake: layer %d is [%d, %d), not a range of midpoint cells 0 <= lo < hi <= %d", l, c0,
                        c1, M);
    }
    const UptLayout U = uptake_layout(h);
    if (U.bins > HC_WTD_HIST_MAX_ENTRIES)
        return fail(HC_ERR_ARG, "root uptake: %lld histogram entries exceed HC_WTD_HIST_MAX_ENTRIES", (long long)U.bins);
    if (int rc = h->upt.ensure(h->n_points, h->n_rows, h->p.dim_d, U.words)) return rc;
    if (h->upt_bins > 0)
        if (int rc = h->uhist.ensure(h->n_points, h->n_rows, h->p.dim_d, U.bins + 2)) return rc;
    if (h->n_members > 0)
        if (int rc = h->uacc.ensure(h->n_members, U.K, 0, h->n_members * U.K)) return rc;
    return HC_OK;
}
int ensure_uptake_hist(hc_handle *h)
{
    if (int rc = ensure_uptake(h)) return rc;
    return h->upt_bins > 0 ? HC_OK : fail(HC_ERR_ARG, "root uptake has no histogram (hc_set_root_uptake with bins = 0)");
}
int ensure_uptake_acc(hc_handle *h)
{
    if (int rc = ensure_uptake(h)) return rc;
    return h->n_members > 0 ? HC_OK : fail(HC_ERR_ARG, "root uptake: no members yet (hc_set_members / hc_set_state)");
}
// the points' midpoint tables on the device, [P][5][D - 1]
int ensure_mid_tabs(hc_handle *h)
{
    if (!h->mid_dirty && h->mid_tabs.p) return HC_OK;
    if (h->mid_tabs.ensure(h->mid_host.size())) return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpy(h->mid_tabs.p, h->mid_host.data(), h->mid_host.size() * 8, hipMemcpyHostToDevice));
    h->mid_dirty = false;
    return HC_OK;
}

// An assimilation table keyed by (points, rows, stride): `per_row` entries per point and analysis row (every stride-th
// row), created on a fresh key as NaN with each slot's count 0 (`width` entries a slot; 0: all NaN)
int ensure_da_table(hc_handle *h, AccTable<double> &t, int64_t stride, int64_t per_row, int width)
{
    const bool fresh = !(t.key[0] == h->n_points && t.key[1] == h->n_rows && t.key[2] == stride);
    const int64_t n = (int64_t)h->n_points * ((h->n_rows - 1) / stride + 1) * per_row;
    if (int rc = t.ensure(h->n_points, h->n_rows, stride, n)) return rc;
    if (fresh) {
        hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, t.buf.p,
                           (size_t)n, width);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return HC_OK;
}

// A record's diagnostics, [P][n_arow][n][6] float64, and a window's, [P][n_arow][n][4], both created as NaN: `owner`
// ensures the filter's own table (ensure_filter, ensure_enkf), `stride` is its stride, `setter` the entry point that
// sets the record or the window
int ensure_record(hc_handle *h, SmRecord &r, int (*owner)(hc_handle *), int64_t stride, const char *setter)
{
    if (r.n <= 0) return fail(HC_ERR_ARG, "no soil-moisture record (%s)", setter);
    if (int rc = owner(h)) return rc;
    if (r.rows != h->n_rows)
        return fail(HC_ERR_ARG, "the soil-moisture record has %lld rows, the forcing %lld: set the record again",
                    (long long)r.rows, (long long)h->n_rows);
    return ensure_da_table(h, r.table, stride, (int64_t)r.n * ENKF_SENSOR_WIDTH, 0);
}
int ensure_window(hc_handle *h, WindowBase &w, int (*owner)(hc_handle *), int64_t stride, const char *setter)
{
    if (w.n <= 0) return fail(HC_ERR_ARG, "no window offsets (%s)", setter);
    if (int rc = owner(h)) return rc;
    return ensure_da_table(h, w.table, stride, (int64_t)w.n * ENKF_WINDOW_WIDTH, 0);
}

// the particle filter's diagnostics (hc_set_filter): [P][n_arow][4] float64, created as count 0 and NaN
int ensure_filter(hc_handle *h)
{
    if (h->filt_stride <= 0) return fail(HC_ERR_ARG, "the particle filter is off (hc_set_filter)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    return ensure_da_table(h, h->filt, h->filt_stride, 4, 4);
}

void filter_shard_off(hc_handle *h)
{
    h->fs_n = h->fs_index = 0;
    h->fs_words = 0;
    h->fs_buf = nullptr;
    h->fs_gather = nullptr;
    h->fs_route = nullptr;
    h->fs_ctx = nullptr;
    h->fs_bounds.clear(); h->fs_counts.clear(); h->fs_send_words.clear(); h->fs_recv_words.clear();
    h->fs_bounds_dev.release(); h->fs_rank.release(); h->fs_table.release(); h->fs_list.release(); h->fs_src.release();
    h->fs_w.release();
}

// The caller's buffer of a shard of n members of a point with n_global, in 8-byte words: the gathered water-table
// indices [n_global], then the send region and the receive region.  The ancestry is monotone, so a shard's slots have
// at most n distinct ancestors elsewhere, and the runs of its own members in the other shards' slots hold at most
// n + S - 1 (two neighbouring destinations may both take the member their runs meet in).
struct FilterShardLayout {
    int64_t send, recv, words;         // the regions' offsets, the total
};
FilterShardLayout filter_shard_layout(int64_t n_global, int64_t n, int64_t S, int64_t D)
{
    FilterShardLayout L;
    L.send = n_global;
    L.recv = L.send + (n + S - 1) * 2 * D;
    L.words = L.recv + n * 2 * D;
    return L;
}

int ensure_fsm(hc_handle *h)
{
    return ensure_record(h, h->filt_sm, ensure_filter, h->filt_stride, "hc_set_filter_soil_moisture");
}

// the table of the tempered weights (hc_set_filter_tempering): [P][n_arow][4] float64, created as NaN
int ensure_ftemp(hc_handle *h)
{
    if (h->filt_floor <= 0.0) return fail(HC_ERR_ARG, "the filter's weights are not tempered (hc_set_filter_tempering)");
    if (int rc = ensure_filter(h)) return rc;
    return ensure_da_table(h, h->ftemp, h->filt_stride, TEMPER_WIDTH, 0);
}

int ensure_fwin(hc_handle *h) { return ensure_window(h, h->filt_win, ensure_filter, h->filt_stride, "hc_set_filter_window"); }

void fwin_off(hc_handle *h)
{
    h->filt_win.clear();
    h->filt_ycols = 0;
    h->fwin_wmax.release();
    if (h->filt_sm.n <= 0) {
        h->filt_qm.release(); h->filt_Y.release(); h->filt_lmax.release(); h->filt_part.release(); h->filt_sums.release();
        h->filt_ipart.release();
    }
}

void temper_off(hc_handle *h)
{
    h->filt_floor = 0.0;
    h->ftemp.release();
    h->filt_trials.release(); h->filt_tstate.release(); h->filt_tpart.release();
}

// the table of the rejuvenation (hc_set_filter_rejuvenation): [P][n_arow][4] float64, created as NaN
int ensure_frej(hc_handle *h)
{
    if (h->rj_delta <= 0.0) return fail(HC_ERR_ARG, "the base vectors are not rejuvenated (hc_set_filter_rejuvenation)");
    if (int rc = ensure_filter(h)) return rc;
    return ensure_da_table(h, h->frej, h->filt_stride, REJUV_WIDTH, 0);
}

void rejuv_off(hc_handle *h)
{
    h->rj_delta = h->rj_a = h->rj_h = 0.0;
    h->frej.release();
    h->rj_part.release(); h->rj_sums.release(); h->rj_mom.release(); h->rj_refused.release();
}

void fsm_off(hc_handle *h)
{
    h->filt_sm.clear();
    h->filt_ycols = 0;
    h->filt_qm.release(); h->filt_Y.release(); h->filt_lmax.release(); h->filt_part.release(); h->filt_sums.release();
    h->filt_ipart.release();
}

// the smoother's tables (hc_set_filter_smoother): shist [P][n_srow][D] int32 zeroed and spaths [P][n_srow][2] int64 as
// (0, -1), and the ring's buffers; on a fresh key (the points, the forcing rows or the depth changed) the ring is emptied
int64_t smoother_rows(const hc_handle *h) { return (h->n_rows - 1) / h->smo_stride + 1; }
int64_t smoother_entries(const hc_handle *h) { return (int64_t)h->n_points * smoother_rows(h) * h->p.dim_d; }
int smoother_paths_init(hc_handle *h)
{
    std::vector<long long> init((size_t)h->smo_paths.n);
    for (size_t k = 0; k < init.size(); k++) init[k] = k % 2 ? -1 : 0;
    HIP_TRY(hipMemcpy(h->smo_paths.buf.p, init.data(), init.size() * 8, hipMemcpyHostToDevice));
    return HC_OK;
}
int ensure_smoother(hc_handle *h)
{
    if (h->smo_stride <= 0) return fail(HC_ERR_ARG, "the filter's smoother is off (hc_set_filter_smoother)");
    if (int rc = ensure_filter(h)) return rc;
    if (smoother_entries(h) > HC_WTD_HIST_MAX_ENTRIES)
        return fail(HC_ERR_ARG, "the filter's smoother: %lld entries exceed HC_WTD_HIST_MAX_ENTRIES (take a longer stride)",
                    (long long)smoother_entries(h));
    const AccTable<int> &t = h->smo_hist;
    const bool fresh = !(t.key[0] == h->n_points && t.key[1] == h->n_rows && t.key[2] == h->p.dim_d);
    if (int rc = h->smo_hist.ensure(h->n_points, h->n_rows, h->p.dim_d, smoother_entries(h))) return rc;
    if (int rc = h->smo_paths.ensure(h->n_points, h->n_rows, h->p.dim_d, (int64_t)h->n_points * smoother_rows(h) * 2))
        return rc;
    const size_t ring = (size_t)(h->smo_lag + 1) * (size_t)h->n_members;
    if (h->smo_w.ensure(ring) || h->smo_w_alt.ensure(ring) || h->smo_id.ensure(ring) || h->smo_id_alt.ensure(ring))
        return HC_ERR_DEVICE;
    if (fresh) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (int rc = smoother_paths_init(h)) return rc;
        h->smo_row.assign((size_t)(h->smo_lag + 1), (int64_t)-1);
        h->smo_last = -1;
    }
    return HC_OK;
}

void smoother_off(hc_handle *h)
{
    h->smo_stride = h->smo_lag = 0;
    h->smo_last = -1;
    h->smo_row.clear();
    h->smo_hist.release(); h->smo_paths.release();
    h->smo_w.release(); h->smo_w_alt.release(); h->smo_id.release(); h->smo_id_alt.release();
}

// what turns the filter off: new points, members or noise source (include/hydrocol.h hc_set_filter)
void filter_off(hc_handle *h)
{
    filter_shard_off(h);
    smoother_off(h);
    fsm_off(h);
    fwin_off(h);
    temper_off(h);
    rejuv_off(h);
    h->filt_stride = 0;
    h->filt_done = false;
    h->filt.release();
    h->psi_alt.release(); h->base_alt.release();
    h->filt_q.release(); h->filt_anc.release(); h->filt_tiles.release(); h->filt_rows.release();
    h->filt_qr.release(); h->filt_surv.release();
}

// the EnKF's diagnostics (hc_set_enkf): [P][n_arow][8] float64, created as count 0 and NaN
int ensure_enkf(hc_handle *h)
{
    if (h->enkf_stride <= 0) return fail(HC_ERR_ARG, "the EnKF is off (hc_set_enkf)");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    return ensure_da_table(h, h->enkf, h->enkf_stride, ENKF_WIDTH, ENKF_WIDTH);
}

// the noise field's diagnostics (hc_set_enkf_noise_field): [P][n_arow][4 D + 1] float64, created as NaN
int ensure_nz(hc_handle *h)
{
    if (!h->enkf_nz) return fail(HC_ERR_ARG, "the noise field is off (hc_set_enkf_noise_field)");
    if (int rc = ensure_enkf(h)) return rc;
    return ensure_da_table(h, h->enkf_nzt, h->enkf_stride, 4 * (int64_t)h->p.dim_d + 1, 0);
}

// the forcing state's diagnostics (hc_set_enkf_forcing): [P][n_arow][9] float64, created as NaN
int ensure_fg(hc_handle *h)
{
    if (!h->enkf_fg) return fail(HC_ERR_ARG, "the forcing analysis is off (hc_set_enkf_forcing)");
    if (int rc = ensure_enkf(h)) return rc;
    return ensure_da_table(h, h->enkf_fgt, h->enkf_stride, ENKF_FORCING_WIDTH, 0);
}

int ensure_sm(hc_handle *h) { return ensure_record(h, h->enkf_sm, ensure_enkf, h->enkf_stride, "hc_set_enkf_soil_moisture"); }
int ensure_win(hc_handle *h) { return ensure_window(h, h->enkf_win, ensure_enkf, h->enkf_stride, "hc_set_enkf_window"); }

void win_off(hc_handle *h)
{
    h->enkf_win.clear();
    h->enkf_eps_w.release();
}

void sm_off(hc_handle *h)
{
    h->enkf_sm.clear();
    h->enkf_eps_s.release();
}

void shard_off(hc_handle *h)
{
    h->shard_global = h->shard_first = h->shard_words = 0;
    h->shard_buf = nullptr;
    h->shard_fn = nullptr;
    h->shard_ctx = nullptr;
    h->enkf_first.release();
}

// what a sharded analysis of a point with n_global members gathers at most, in doubles: the global tile count times the
// widest pass as the record and the window stand -- the prior products with the squared psi anomalies the relaxation
// takes along, or the posterior's
int64_t shard_words_needed(const hc_handle *h, int64_t n_global)
{
    const int64_t D = h->p.dim_d, Wx = 1 + h->enkf_sm.n + h->enkf_win.n, n_tiles = (n_global + ENKF_TILE - 1) / ENKF_TILE;
    return n_tiles * std::max((D + Wx) * Wx + D, (Wx + 1) * (Wx + 1));
}

void nz_off(hc_handle *h)
{
    h->enkf_nz = h->nz_done = false;
    h->enkf_nz_alpha = 0.0;
    h->enkf_nzt.release();
    h->enkf_z.release(); h->nz_rej.release(); h->nz_rejsum.release();
}

void fg_off(hc_handle *h)
{
    h->enkf_fg = h->fg_done = false;
    h->enkf_fg_alpha = 0.0;
    h->enkf_fgt.release();
    h->enkf_gv.release(); h->fg_x.release(); h->fg_rej.release(); h->fg_rejsum.release();
}

void enkf_off(hc_handle *h)
{
    shard_off(h);
    nz_off(h);
    fg_off(h);
    h->enkf_stride = 0;
    h->enkf_done = false;
    h->enkf_width = 0;
    h->enkf.release();
    h->enkf_Y.release(); h->enkf_eps.release(); h->enkf_Ypost.release(); h->enkf_part.release();
    h->enkf_part_sq.release(); h->enkf_psi.release();
    h->enkf_method = 0;
    h->enkf_alpha = 0.0;
    h->enkf_last_method = 0;
    h->enkf_last_relaxed = false;
    sm_off(h);
    win_off(h);
}

// the Philox source's vectors are white again (hc_set_noise_correlation)
void noise_corr_off(hc_handle *h)
{
    h->ncorr = false;
    h->ncorr_ab.clear();
    h->ncorr_dev.release();
}

// A Philox run's caller-style vectors [n_vec][N][D] from the kernel's own normals: the base vectors times the members'
// scales (rows == NULL, n_vec = 1) or the refresh rows rows[v]; correlated down the column when a correlation is set.
int launch_noise_fill(hc_handle *h, double *out, int64_t n_vec, const long long *rows, const double *nscale)
{
    const long long N = h->n_members, mpp = N / h->n_points;
    const int D = h->p.dim_d;
    const long long *point_base = h->n_points > 1 ? h->point_base.p : nullptr;
    if (h->ncorr) {
        const size_t items = (size_t)n_vec * h->n_points * (size_t)((mpp + NF_TILE - 1) / NF_TILE);
        if (items > (size_t)INT32_MAX)           // (one block per item; the 4 GiB a launch stages hold far fewer)
            return fail(HC_ERR_ARG, "noise field: %zu tiles in one fill exceed 2^31 - 1", items);
        hipLaunchKernelGGL(noise_field_fill_kernel, dim3((unsigned)items), dim3(NF_THREADS), 0, h->stream, out,
                           (long long)n_vec, rows, h->draw_idx.p, (unsigned long long)h->seed, (long long)h->member_offset,
                           point_base, mpp, N, D, nscale, h->ncorr_dev.p, h->ncorr_dev.p + (size_t)h->n_points * D);
        return HC_OK;
    }
    const size_t cnt = (size_t)n_vec * N * D;
    const unsigned blocks = (unsigned)std::min<size_t>((cnt + 255) / 256, (size_t)h->n_cu * 64);
    hipLaunchKernelGGL(filter_philox_fill_kernel, dim3(blocks), dim3(256), 0, h->stream, out, (long long)n_vec, rows,
                       h->draw_idx.p, (unsigned long long)h->seed, (long long)h->member_offset, point_base, mpp, N, D, nscale);
    return HC_OK;
}

// what turns both filters and the noise correlation off: new points, members or noise source (include/hydrocol.h
// hc_set_filter, hc_set_enkf, hc_set_noise_correlation)
void forcing_pert_off(hc_handle *h)
{
    fg_off(h);                   // (the state the EnKF would analyse goes with it)
    h->fp_on = false;
    h->fp_day = h->fp_day_next = h->fp_offset = -1;
    h->fp_g.release(), h->fp_g_alt.release(), h->fp_fmul.release();
}

// the global id of the handle's first member: the one given, else the Philox source's, else (host noise) 0
long long forcing_member_offset(const hc_handle *h)
{
    return h->fp_offset >= 0 ? h->fp_offset : (h->philox ? h->member_offset : 0);
}

ForcingPert forcing_pert_of(const hc_handle *h)
{
    ForcingPert F;
    for (int s = 0; s < 2; s++) {
        F.sigma[s] = h->fp_sigma[s];
        F.half[s] = h->fp_sigma[s] * h->fp_sigma[s] / 2.0;
    }
    F.phi = h->fp_phi;
    F.c = h->fp_c;
    F.seed = h->fp_seed;
    return F;
}

// The factors of the days rows [row0, row0 + rows) touch -> fp_fmul [n_days][2][N], the state advanced to the last of them
// in the second buffer (forcing_fill_commit takes it over once the step launch is issued: a launch that fails leaves the
// state where it stood); IoArgs told where they are.  (fill_args has uploaded the points' keys.)
int launch_forcing_fill(hc_handle *h, int64_t row0, int64_t rows)
{
    const long long N = h->n_members, day0 = row0 / HC_FORCING_DAY_ROWS, day1 = (row0 + rows - 1) / HC_FORCING_DAY_ROWS;
    if (h->fp_day > day0)
        return fail(HC_ERR_ARG, "perturbed forcing: row %lld lies in day %lld, behind day %lld the members' state stands at "
                                "(hc_set_forcing_state or hc_set_forcing_perturbation rewinds it)", (long long)row0, day0,
                    (long long)h->fp_day);
    if (day1 > (long long)UINT32_MAX) return fail(HC_ERR_ARG, "perturbed forcing: day %lld exceeds 2^32 - 1", day1);
    if (h->fp_g.ensure((size_t)(2 * N)) || h->fp_g_alt.ensure((size_t)(2 * N)) ||
        h->fp_fmul.ensure((size_t)((day1 - day0 + 1) * 2 * N)))
        return HC_ERR_DEVICE;
    hipLaunchKernelGGL(forcing_factor_fill_kernel, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, h->stream, h->fp_g.p,
                       h->fp_g_alt.p, (long long)h->fp_day, N, h->fp_fmul.p, 0LL, N, day0, day1, N / h->n_points,
                       h->n_points > 1 ? h->point_base.p : nullptr, forcing_member_offset(h), forcing_pert_of(h));
    HIP_TRY(hipGetLastError());
    h->fp_day_next = day1;
    h->io_host.fmul = h->fp_fmul.p;
    h->io_host.fmul_day0 = day0;
    return HC_OK;
}

void forcing_fill_commit(hc_handle *h)
{
    if (h->fp_day_next < 0) return;
    std::swap(h->fp_g, h->fp_g_alt);
    h->fp_day = h->fp_day_next;
    h->fp_day_next = -1;
}

void assimilation_off(hc_handle *h)
{
    filter_off(h);
    enkf_off(h);
    noise_corr_off(h);
}

// The filter that is on (the particle filter and the EnKF exclude each other): its stride (0: neither), its record and
// window, what ensures their tables, and its analysis rows (every stride-th row)
struct Assim {
    int64_t stride;
    const SmRecord &sm;
    const WindowBase &win;
    int (*ensure_sm)(hc_handle *), (*ensure_win)(hc_handle *);
};
Assim assim(const hc_handle *h)
{
    if (h->filt_stride > 0) return {h->filt_stride, h->filt_sm, h->filt_win, ensure_fsm, ensure_fwin};
    return {h->enkf_stride, h->enkf_sm, h->enkf_win, ensure_sm, ensure_win};
}
int64_t assim_rows(const hc_handle *h) { return (h->n_rows - 1) / assim(h).stride + 1; }

// The bodies of the table entry points: the table as `ensure` leaves it (its rules and refusals), a size check when the
// caller names one (n >= 0), the stream drained, one copy of the whole table: host -> table, table -> host or
// table -> device memory elsewhere (`kind`).
template <typename T>
int table_copy(hc_handle *h, AccTable<T> &t, int (*ensure)(hc_handle *), hipMemcpyKind kind, void *other, int64_t n = -1,
               const char *who = nullptr)
{
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure(h)) return rc;
    if (n >= 0 && n != t.n)
        return fail(HC_ERR_ARG, "%s: the table has %lld %s, not %lld", who, (long long)t.n, t.unit, (long long)n);
    HIP_TRY(hipStreamSynchronize(h->stream));
    const bool in = kind == hipMemcpyHostToDevice;
    HIP_TRY(hipMemcpy(in ? (void *)t.buf.p : other, in ? other : (void *)t.buf.p, (size_t)t.n * sizeof(T), kind));
    if (kind == hipMemcpyDeviceToDevice) HIP_TRY(hipDeviceSynchronize());
    return HC_OK;
}
template <typename T>
int table_reset(hc_handle *h, AccTable<T> &t, int (*ensure)(hc_handle *))
{
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    t.invalidate();
    return ensure(h);
}

int push_io(hc_handle *h)
{
    HIP_TRY(hipMemcpyAsync(h->iodev.p, &h->io_host, sizeof(IoArgsExt), hipMemcpyHostToDevice, h->stream));
    return HC_OK;
}

int fill_args(hc_handle *h, StepArgs &A)
{
    if (!h->have_column) return fail(HC_ERR_ARG, "hc_set_column has not been called");
    if (!h->have_forcing) return fail(HC_ERR_ARG, "hc_set_forcing has not been called");
    if (h->n_members <= 0 || !h->psi.p) return fail(HC_ERR_ARG, "hc_set_members / hc_set_state has not been called");
    if (!h->have_noise) return fail(HC_ERR_ARG, "no noise source: call hc_set_noise_host or hc_set_noise_philox");
    memset(&A, 0, sizeof(A));
    IoArgsExt &io = h->io_host;
    memset(&io, 0, sizeof(io));
    const int NP = h->n_points;
    if (h->n_members % NP != 0)
        return fail(HC_ERR_ARG, "%lld members do not divide into %d parameter points", (long long)h->n_members, NP);
    if (h->Pdev.ensure((size_t)NP) || h->iodev.ensure(1)) return HC_ERR_DEVICE;
    if (h->points_dirty) {
        if (h->tab.ensure(h->tab_host.size()) || h->node_tabs.ensure(h->node_host.size())) return HC_ERR_DEVICE;
        HIP_TRY(hipMemcpy(h->tab.p, h->tab_host.data(), h->tab_host.size() * 8, hipMemcpyHostToDevice));
        if (h->pair_ok) {
            if (h->tab_pair.ensure(h->tab_pair_host.size())) return HC_ERR_DEVICE;
            HIP_TRY(hipMemcpy(h->tab_pair.p, h->tab_pair_host.data(), h->tab_pair_host.size() * 8, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipMemcpy(h->node_tabs.p, h->node_host.data(), h->node_host.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->Pdev.p, h->P_host.data(), (size_t)NP * sizeof(ColumnDev), hipMemcpyHostToDevice));
        {   // the reciprocal table is the device's own arithmetic (hc_device.h T_RDELTA)
            const int S1 = WAVE * h->cpl;
            hipLaunchKernelGGL(fill_rdelta, dim3((unsigned)NP), dim3(256), 0, h->stream, h->tab.p, h->Pdev.p, S1);
            if (h->pair_ok)
                hipLaunchKernelGGL(fill_rdelta, dim3((unsigned)NP), dim3(256), 0, h->stream, h->tab_pair.p, h->Pdev.p, 2 * WAVE * PAIR_CPL);
#if (HC_CPL_MASK >> 5) & 1
            if (h->cpl == KSAT_CPL)      // ... and so is a saturated cell's K (T_KSAT; it reads T_RDELTA)
                HIP_TRY(launch_fill_ksat(h->stream, h->tab.p, h->Pdev.p, NP));
#endif
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        h->points_dirty = false;
    }
    if (int rc = ensure_moments(h)) return rc;
    A.n_points = NP;
    A.members_per_point = h->n_members / NP;
    {
        // chunks of one point's members for the multi-point scheduler: >= 8 chunks per workgroup when the ensemble
        // allows it, <= 32 members per wave (that bounds the idle time at a chunk's end to ~1.5 %) and never fewer
        // members than the workgroup has waves
        // members a workgroup advances at once: its waves, or its pairs of waves on the split column
        const long long waves = h->use_pair() ? wpb_of(PAIR_CPL, 2) / 2 : wpb_of(h->cpl, 1, h->use_special());
        long long chunk = h->chunk_members > 0 ? h->chunk_members : (h->n_members + 8LL * h->n_cu - 1) / (8LL * h->n_cu);
        chunk = std::max<long long>(waves, std::min<long long>(chunk, 32 * waves));
        chunk = std::min<long long>(chunk, A.members_per_point);
        A.chunk_members = (int)chunk;
        A.chunks_per_point = (int)((A.members_per_point + chunk - 1) / chunk);
        A.n_chunks = A.chunks_per_point * NP;
    }
    {
        // deep columns: room for the per-wave vectors LDS cannot hold, for every wave of the persistent grid
        const size_t per_wave = std::max(std::max((size_t)spill_doubles(h->cpl, 1, true), (size_t)spill_doubles(h->cpl, 1, false)),
                                         (size_t)spill_doubles(PAIR_CPL, 2));
        const size_t cnt = (size_t)h->n_cu * MAX_WAVES_PER_BLOCK * per_wave;
        if (h->wave_spill.ensure(cnt)) return HC_ERR_DEVICE;
        A.wave_spill = h->wave_spill.p;
    }
    A.P = h->Pdev.p;
    A.io = h->iodev.p;
    A.tab = h->tab.p;          // (launch_step switches to the split-column tables)
    A.gtab = h->gtab.p;
    A.n_members = h->n_members;
    A.D = h->P.D;
    A.n_groups = h->p.n_groups;
    A.host_noise = h->philox && !h->noise_host() ? 0 : 1;   // a filtered Philox run hands its normals over as caller noise
    A.psi_sat = h->P.psi_sat;
    A.jac_reject = h->jac_reject;
    A.max_phase_iterations = h->max_phase_iterations;
    A.scipy_152 = h->scipy_152;
    io.psi = h->psi.p;
    io.base_noise = A.host_noise ? h->base.p : nullptr;
    io.nscale = h->nscale.p;
    io.precip = h->precip.p;
    io.atm = h->atm.p;
    io.daylight = h->daylight.p;
    io.refresh = h->refresh.p;
    io.wtd_obs = h->wtd_obs.p;
    io.draw_idx = h->draw_idx.p;
    io.member_offset = h->member_offset;
    io.seed = h->seed;
    io.counters = h->counters.p;
    io.queue = h->counters.p + 63;
    if (NP > 1) {
        if (h->point_base.ensure((size_t)NP) || h->point_order.ensure((size_t)NP) || h->point_cost.ensure((size_t)NP))
            return HC_ERR_DEVICE;
        std::vector<long long> base(h->base_host);
        if ((int)base.size() != NP) {
            base.resize((size_t)NP);
            for (int k = 0; k < NP; k++) base[(size_t)k] = h->member_offset + (long long)k * A.members_per_point;
        }
        if ((int)h->order_host.size() != NP) {
            h->order_host.resize((size_t)NP);
            for (int k = 0; k < NP; k++) h->order_host[(size_t)k] = k;
        }
        if ((int)h->cost_total.size() != NP) h->cost_total.assign((size_t)NP, 0ull);
        HIP_TRY(hipMemcpy(h->point_base.p, base.data(), (size_t)NP * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->point_order.p, h->order_host.data(), (size_t)NP * 4, hipMemcpyHostToDevice));
        io.point_base = h->point_base.p;
        io.point_order = h->point_order.p;
        io.point_cost = h->point_cost.p;
    }
#ifdef HC_PROFILE
    if (getenv("HYDROCOL_DEBUG_TRACE")) {
        if (h->trace.ensure((size_t)1 + 6 * HC_TRACE_N)) return HC_ERR_DEVICE;
        hipMemset(h->trace.p, 0, ((size_t)1 + 6 * HC_TRACE_N) * 8);
        io.trace = h->trace.p;
    }
#endif
    return HC_OK;
}

}  // namespace

// ------------------------------------------------------------------ C-ABI
extern "C" {

const char *hc_last_error(void) { return g_err.c_str(); }
#ifndef HC_KERNEL_HASH
#define HC_KERNEL_HASH "unknown"
#endif
// "... kernels <hash>": identity of the device code (sources + compile flags + compiler, __graft_entry__.kernel_hash)
const char *hc_version(void) { return "hydrocol 0.4 (gfx950) kernels " HC_KERNEL_HASH; }

int hc_create(int device_ordinal, hc_handle **out)
{
    if (!out) return fail(HC_ERR_ARG, "hc_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(HC_ERR_NO_DEVICE, "no HIP device visible (%s): the hydrocol stepper has no CPU path",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= count)
        return fail(HC_ERR_ARG, "device ordinal %d out of range [0,%d)", device_ordinal, count);
    HIP_TRY(hipSetDevice(device_ordinal));
    hc_handle *h = new hc_handle();
    h->device = device_ordinal;
    // everything acquired so far is released when a later step fails
    auto init = [&]() -> int {
        HIP_TRY(hipStreamCreate(&h->stream));
        HIP_TRY(hipEventCreate(&h->ev0));
        HIP_TRY(hipEventCreate(&h->ev1));
        if (h->counters.ensure(128) != HC_OK) return HC_ERR_DEVICE;
        HIP_TRY(hipMemset(h->counters.p, 0, 128 * sizeof(unsigned long long)));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device_ordinal));
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (const char *e = getenv("HYDROCOL_DEBUG_CUS"))      // measurement hook: a smaller persistent grid
            if (atoi(e) > 0) h->n_cu = std::min(h->n_cu, atoi(e));
        return HC_OK;
    };
    if (const int rc = init()) {
        const std::string keep = g_err;
        hc_destroy(h);
        g_err = keep;
        return rc;
    }
    if (const char *cm = getenv("HYDROCOL_CHUNK_MEMBERS"))
        if (atoi(cm) > 0) h->chunk_members = atoi(cm);
    const char *rpl = getenv("HYDROCOL_ROWS_PER_LAUNCH");
    if (rpl && atoi(rpl) > 0) h->rows_per_launch = atoi(rpl);
    if (const char *sg = getenv("HYDROCOL_STRICT_GUARD")) h->strict_guard = atoi(sg) != 0;
    if (const char *po = getenv("HYDROCOL_POINT_ORDER")) h->fixed_order = strcmp(po, "fixed") == 0;
    if (const char *sc = getenv("HYDROCOL_SPLIT_COLUMN")) {
        h->no_split = atoi(sc) == 0;
        h->force_split = atoi(sc) == 1;
    }
    if (const char *mp = getenv("HYDROCOL_MODEL_PACK")) h->model_pack = atoi(mp) != 0;
    if (const char *j3 = getenv("HYDROCOL_JAC_LOCAL3")) h->jac_local3 = atoi(j3) != 0;
    if (const char *sv = getenv("HYDROCOL_SCIPY_152")) h->scipy_152 = atoi(sv) != 0;     // (the whole product at once: CLI, Simulation)
    if (const char *mi = getenv("HYDROCOL_DEBUG_MAX_ITER"))    // test hook: forces abandoned attempts
        if (atoi(mi) > 0) h->max_phase_iterations = atoi(mi);
    if (const char *cc = getenv("HYDROCOL_COV_CHUNK_MEMBERS"))        // test hook: the theta covariance's members in chunks
        if (atoi(cc) > 0) h->cov_chunk = atoi(cc);
    if (const char *gy = getenv("HYDROCOL_DEBUG_STORAGE_GRID_Y"))     // test hook: blocks of layer_storage_kernel take several slices
        if (atoi(gy) > 0) h->stor_grid_y = std::min(h->stor_grid_y, (long long)atoi(gy));
    const char *jr = getenv("HYDROCOL_DEBUG_JAC_REJECT");   // test hook: exercises num_jac's retry branch
    if (jr && atof(jr) > 0.0) h->jac_reject = atof(jr);
    *out = h;
    return HC_OK;
}

int hc_destroy(hc_handle *h)
{
    if (!h) return HC_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->tab.release(); h->node_tabs.release(); h->precip.release(); h->atm.release(); h->psi.release();
    h->base.release(); h->nscale.release(); h->fresh.release(); h->psi_rows.release(); h->scratch_d.release();
    h->diag.release();
    h->wave_spill.release();
    h->spin_iters.release();
    h->trace.release();
    h->tab_pair.release(); h->gtab_pair.release();
    h->gtab.release(); h->wtd_obs.release(); h->draw_idx.release(); h->stats.release(); h->scratch_i.release();
    h->Pdev.release(); h->iodev.release();
    h->point_base.release(); h->point_order.release(); h->point_cost.release();
    h->daylight.release(); h->refresh.release(); h->wtd_u16.release(); h->moments.release(); h->counters.release();
    h->prof.release(); h->hist.release(); h->thist.release(); h->stor.release(); h->shist.release();
    h->cov.release(); h->cov_q.release();
    h->cond.release();
    h->pacc.release(); h->pacc_alt.release(); h->pmom.release(); h->phist.release();
    uptake_off(h);
    assimilation_off(h);
    forcing_pert_off(h);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return HC_OK;
}

// One parameter point: ColumnDev + the slot tables of the stepper.  `first` fixes the geometry shared by all points.
static int build_point(hc_handle *h, const hc_column_params *p, const double *node_tabs, const double *mid_tabs,
                       bool first)
{
    const int D = p->dim_d;
    if (!(p->dz > 0.0) || !(p->n > 1.0) || !(p->alpha > 0.0)) return fail(HC_ERR_ARG, "bad dz / n / alpha");
    if (p->n_root_first < 0 || p->n_root_first > 1 || p->n_root_int < 0 || p->n_root_int > D - 2)
        return fail(HC_ERR_ARG, "bad root-zone cell counts");
    if (!first && (D != h->p.dim_d || p->n_groups != h->p.n_groups || p->dz != h->p.dz))
        return fail(HC_ERR_ARG, "a parameter point must share dim_d, n_groups and dz with point 0");
    // low_lim = k - (sat_cells - 1) must stay inside the k-cell slice pde_fun sees: sat_cells >= 1
    if (p->flag_predict && p->sat_cells < 1) return fail(HC_ERR_ARG, "PREDICT mode: sat_cells = %d, must be >= 1", p->sat_cells);
    // delta = por - theta_res divides the effective saturation: with delta <= 0 a saturated cell would silently get K = 0
    for (int i = 0; i < D; i++)
        if (!(node_tabs[i] > p->theta_res))
            return fail(HC_ERR_ARG, "node %d: porosity %g is not above theta_res = %g", i, node_tabs[i], p->theta_res);
    for (int i = 0; i < D - 1; i++)
        if (!(mid_tabs[i] > p->theta_res))
            return fail(HC_ERR_ARG, "cell %d: porosity %g is not above theta_res = %g", i, mid_tabs[i], p->theta_res);
    ColumnDev P{};
    P.D = D; P.model = p->model; P.flag_et = p->flag_et; P.flag_lf = p->flag_lf; P.flag_hlift = p->flag_hlift;
    P.n_root_first = p->n_root_first; P.n_root_int = p->n_root_int;
    P.theta_res = p->theta_res; P.alpha = p->alpha; P.n = p->n; P.m = p->m; P.psi_sat = p->psi_sat;
    P.epsilon = p->epsilon; P.lambda = p->lambda_exp; P.sigma = p->sigma_noise; P.sat_soil = p->sat_soil;
    P.dz = p->dz; P.inv_dz = 1.0 / p->dz; P.ipsi50 = p->ipsi50; P.lai = p->lai; P.surface_evap = p->surface_evap;
    P.interception = p->interception; P.evap_delta_min = p->evap_delta_min;
    P.mn_alpha = (p->m * p->n) * p->alpha;
    P.inv_m = 1.0 / p->m;
    P.por_node0 = node_tabs[0];
    // repaired PREDICT mode: low_lim = dim_d - (sat_cells - 1) of each pde_fun call as an int, nothing drains when
    // it is not positive (the reference's np.linspace(1.5, 0.0, low_lim) raises for a float or a negative count)
    P.flag_predict = p->flag_predict ? 1 : 0;
    P.predict_low = std::min(D - 2, std::max(0, (D - 2) - (p->sat_cells - 1)));
    P.predict_first = (1 - (p->sat_cells - 1)) >= 1 ? 1 : 0;
    P.flag_pack = h->model_pack ? 1 : 0;
    P.flag_jac3 = h->jac_local3 ? 1 : 0;

    const int M = D - 1;
    // Slot tables for `halves` waves per member with `cpl` nodes per lane: node / midpoint i sits with wide lane
    // wl = i / cpl, cell c = i % cpl, i.e. in wave wl / 64, slot c * 64 + wl % 64 of that wave's 64 cpl slots.
    auto layout = [&](int cpl, int halves, std::vector<double> &tab) {
        const int SW = WAVE * cpl, S = SW * halves;
        tab.assign((size_t)NTAB * S, 0.0);
        auto put = [&](int slot, double por, double fc, double wlt, double root, double meank, double noisec) {
            const double mk = meank == 0.0 ? 1.0e-7 : meank;   // utilities.py:50
            tab[(size_t)T_POR * S + slot] = por;
            tab[(size_t)T_FC * S + slot] = fc;
            tab[(size_t)T_WLT * S + slot] = wlt;
            tab[(size_t)T_ROOT * S + slot] = root;
            tab[(size_t)T_LOGM * S + slot] = std::log(mk);
            tab[(size_t)T_INVM2 * S + slot] = 1.0 / (mk * mk);
            tab[(size_t)T_NOISEC * S + slot] = noisec;
            tab[(size_t)T_VALID * S + slot] = 1.0;
            const double d1 = por - wlt;                       // tree_roots.py:235-238
            tab[(size_t)T_INVD1 * S + slot] = 1.0 / (d1 == 0.0 ? 1.0 : d1);
        };
        for (int wl = 0; wl < WAVE * halves; wl++)
            for (int c = 0; c < cpl; c++) {
                const int i = wl * cpl + c, slot = (wl / WAVE) * SW + c * WAVE + wl % WAVE;
                if (i < M)
                    put(slot, mid_tabs[i], mid_tabs[M + i], mid_tabs[2 * M + i], mid_tabs[3 * M + i],
                        mid_tabs[4 * M + i], mid_tabs[5 * M + i]);
                else
                    put(slot, 0.3, 0.2, 0.1, 0.0, 1.0, 0.0);    // padding cell: benign, results masked
                if (i >= M) tab[(size_t)T_VALID * S + slot] = 0.0;
            }
        // virtual top-node cell in the always-free last slot of the last lane (of the last wave)
        const int top = (halves - 1) * SW + (cpl - 1) * WAVE + (WAVE - 1);
        put(top, node_tabs[0], 0.2, 0.1, 0.0, node_tabs[D + 0], node_tabs[2 * D + 0]);
        tab[(size_t)T_VALID * S + top] = 0.0;                   // its C / flux never enter the assembly
    };
    std::vector<double> tab;
    layout(h->cpl, 1, tab);
    for (double v : tab)
        if (!std::isfinite(v)) return fail(HC_ERR_ARG, "a column table entry is not finite");
    // split column: 513..640 nodes, the root zone (cells 1..n_root_int) of EVERY point inside the upper half; each point
    // brings its own tables in the two-halves layout (round 4: sweeps at these depths run on the split column too)
    const bool pair_here = D > WAVE * 8 && D <= 2 * WAVE * PAIR_CPL && p->n_root_int <= WAVE * PAIR_CPL - 1;
    if (first) {
        h->pair_ok = pair_here;
        h->tab_pair_host.clear();
    } else {
        h->pair_ok = h->pair_ok && pair_here;
    }
    if (h->pair_ok) {
        std::vector<double> tp;
        layout(PAIR_CPL, 2, tp);
        h->tab_pair_host.insert(h->tab_pair_host.end(), tp.begin(), tp.end());
    }
    const bool special = (p->model == HC_MODEL_VRETTAS_FUNG && p->n == 2.0 && p->m == 0.5 && p->lambda_exp == 1.0);
    if (first) {
        h->P_host.clear(); h->tab_host.clear(); h->node_host.clear();
        h->base_host.clear(); h->order_host.clear(); h->cost_total.clear();
        h->n_points = 0;
        h->p = *p;
        h->P = P;
        h->special = special;
    } else {
        h->special = h->special && special;
    }
    if (h->filt_stride > 0 || h->enkf_stride > 0 || h->ncorr) {   // the points change: the filters are off
        (void)hipStreamSynchronize(h->stream);
        assimilation_off(h);
    }
    if (h->fp_on) {              // ... and so is the perturbed forcing (its state is the members' of the old points)
        (void)hipStreamSynchronize(h->stream);
        forcing_pert_off(h);
    }
    if (first) {                 // a new column: the root uptake (hc_set_root_uptake) is off
        if (h->upt_layers > 0) (void)hipStreamSynchronize(h->stream);
        uptake_off(h);
        h->mid_host.clear();
    }
    // the midpoint tables the root uptake reads, as received, and 1 / (por - wlt) as the slot tables have it
    // (UPT_TAB_*: porosity, field capacity, wilting point, the reciprocal, root density)
    h->mid_host.insert(h->mid_host.end(), mid_tabs, mid_tabs + (size_t)3 * M);
    for (int i = 0; i < M; i++) {
        const double d1 = mid_tabs[i] - mid_tabs[2 * M + i];                   // tree_roots.py:235-238
        h->mid_host.push_back(1.0 / (d1 == 0.0 ? 1.0 : d1));
    }
    h->mid_host.insert(h->mid_host.end(), mid_tabs + (size_t)3 * M, mid_tabs + (size_t)4 * M);
    h->mid_dirty = true;
    h->P_host.push_back(P);
    h->tab_host.insert(h->tab_host.end(), tab.begin(), tab.end());
    h->node_host.insert(h->node_host.end(), node_tabs, node_tabs + (size_t)3 * D);
    h->n_points++;
    h->points_dirty = true;
    return HC_OK;
}

int hc_set_column(hc_handle *h, const hc_column_params *p, const double *node_tabs, const double *mid_tabs,
                  const int32_t *groups)
{
    if (!h || !p || !node_tabs || !mid_tabs || !groups) return fail(HC_ERR_ARG, "hc_set_column: NULL argument");
    const int D = p->dim_d;
    if (D < 4 || D > HC_MAX_DEPTH_NODES) return fail(HC_ERR_ARG, "dim_d = %d outside [4, %d]", D, HC_MAX_DEPTH_NODES);
    if (p->n_groups < 1 || p->n_groups > 16) return fail(HC_ERR_ARG, "n_groups = %d outside [1,16]", p->n_groups);
    for (int i = 0; i < D; i++)
        if (groups[i] < 0 || groups[i] >= p->n_groups) return fail(HC_ERR_ARG, "groups[%d] out of range", i);
    HIP_TRY(hipSetDevice(h->device));
    int cpl = (D + WAVE - 1) / WAVE;
    if (cpl < 2) cpl = 2;
    h->cpl = cpl;
    h->wpb = 4;
    h->slots = WAVE * cpl;
    h->have_column = false;
    int rc = build_point(h, p, node_tabs, mid_tabs, true);
    if (rc) return rc;
    auto group_layout = [&](int cpl_, int halves, std::vector<int> &gt) {
        const int SW = WAVE * cpl_, S = SW * halves;
        gt.assign((size_t)NGTAB * S, -1);
        for (int wl = 0; wl < WAVE * halves; wl++)
            for (int c = 0; c < cpl_; c++) {
                const int i = wl * cpl_ + c, slot = (wl / WAVE) * SW + c * WAVE + wl % WAVE;
                if (i < D) {
                    gt[(size_t)G_SELF * S + slot] = groups[i];
                    gt[(size_t)G_PREV * S + slot] = i >= 1 ? groups[i - 1] : -1;
                    gt[(size_t)G_NEXT * S + slot] = i < D - 1 ? groups[i + 1] : -1;
                }
            }
    };
    std::vector<int> gt;
    group_layout(cpl, 1, gt);
    if (h->gtab.ensure(gt.size())) return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpy(h->gtab.p, gt.data(), gt.size() * 4, hipMemcpyHostToDevice));
    if (h->pair_ok) {
        group_layout(PAIR_CPL, 2, gt);
        if (h->gtab_pair.ensure(gt.size())) return HC_ERR_DEVICE;
        HIP_TRY(hipMemcpy(h->gtab_pair.p, gt.data(), gt.size() * 4, hipMemcpyHostToDevice));
    }
    h->have_column = true;
    return HC_OK;
}

int hc_add_point(hc_handle *h, const hc_column_params *p, const double *node_tabs, const double *mid_tabs)
{
    if (!h || !p || !node_tabs || !mid_tabs) return fail(HC_ERR_ARG, "hc_add_point: NULL argument");
    if (!h->have_column) return fail(HC_ERR_ARG, "hc_set_column (point 0) must come first");
    return build_point(h, p, node_tabs, mid_tabs, false);
}

int hc_get_point_count(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "NULL handle");
    return h->n_points;
}

int hc_set_forcing(hc_handle *h, int64_t n_rows, const double *precip, const double *atm,
                   const uint8_t *daylight, const int32_t *wtd_obs, const uint8_t *refresh)
{
    if (!h || n_rows < 1 || !precip || !atm || !daylight || !wtd_obs || !refresh)
        return fail(HC_ERR_ARG, "hc_set_forcing: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (h->fp_on) {              // another record: the perturbed forcing is off
        HIP_TRY(hipStreamSynchronize(h->stream));
        forcing_pert_off(h);
    }
    const size_t T = (size_t)n_rows;
    // A skipped row (wtd_obs < 0) consumes no noise draw: the reference `continue`s before drawing
    // (simulation.py:582-588 come before :599-602), so its refresh flag is dropped here for everybody downstream.
    std::vector<unsigned char> refresh_eff(refresh, refresh + T);
    for (size_t i = 0; i < T; i++)
        if (wtd_obs[i] < 0) refresh_eff[i] = 0;
    refresh = refresh_eff.data();
    std::vector<int> draw(T, 0);
    int cnt = 0;
    for (size_t i = 0; i < T; i++) {
        if (refresh[i]) cnt++;
        draw[i] = cnt;
    }
    if (h->precip.ensure(T) || h->atm.ensure(T) || h->daylight.ensure(T) || h->refresh.ensure(T) ||
        h->wtd_obs.ensure(T) || h->draw_idx.ensure(T))
        return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpy(h->precip.p, precip, T * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->atm.p, atm, T * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->daylight.p, daylight, T, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->refresh.p, refresh, T, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->wtd_obs.p, wtd_obs, T * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->draw_idx.p, draw.data(), T * 4, hipMemcpyHostToDevice));
    h->h_refresh.assign(refresh, refresh + T);
    h->h_wtd_obs.assign(wtd_obs, wtd_obs + T);
    h->h_daylight.assign(daylight, daylight + T);
    h->n_rows = n_rows;
    h->moments.invalidate();     // (re)allocated and zeroed by the next call that needs the moment tables
    h->have_forcing = true;
    return HC_OK;
}

int hc_set_forcing_row(hc_handle *h, int64_t row, double precip, double atm, uint8_t daylight, int32_t wtd_obs)
{
    if (!h || !h->have_forcing) return fail(HC_ERR_ARG, "hc_set_forcing_row: hc_set_forcing has not been called");
    if (row < 0 || row >= h->n_rows) return fail(HC_ERR_ARG, "hc_set_forcing_row: row %lld outside [0, %lld)", (long long)row,
                                                 (long long)h->n_rows);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const unsigned char zero = 0;
    HIP_TRY(hipMemcpy(h->precip.p + row, &precip, 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->atm.p + row, &atm, 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->daylight.p + row, &daylight, 1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->wtd_obs.p + row, &wtd_obs, 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->refresh.p + row, &zero, 1, hipMemcpyHostToDevice));
    h->h_refresh[(size_t)row] = 0;
    h->h_wtd_obs[(size_t)row] = wtd_obs;
    h->h_daylight[(size_t)row] = daylight;
    return HC_OK;
}

int hc_set_members(hc_handle *h, int64_t n_members)
{
    if (!h || n_members < 1) return fail(HC_ERR_ARG, "hc_set_members: bad argument");
    if (!h->have_column) return fail(HC_ERR_ARG, "hc_set_column must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    assimilation_off(h);
    forcing_pert_off(h);         // the perturbed forcing's state is the members': off
    uptake_off(h);               // the root uptake's accumulators are the members': off
    const size_t n = (size_t)n_members * h->p.dim_d;
    if (h->psi.ensure(n) || h->nscale.ensure((size_t)n_members)) return HC_ERR_DEVICE;
    hipLaunchKernelGGL(fill_d, dim3((unsigned)((n_members + 255) / 256)), dim3(256), 0, h->stream, h->nscale.p, 1.0,
                       (size_t)n_members);
    HIP_TRY(hipGetLastError());
    h->n_members = n_members;
    h->have_noise = false;
    return HC_OK;
}

int hc_set_state(hc_handle *h, const double *psi, int broadcast)
{
    if (!h || !psi) return fail(HC_ERR_ARG, "hc_set_state: bad argument");
    if (h->n_members <= 0) return fail(HC_ERR_ARG, "hc_set_members must come first");
    HIP_TRY(hipSetDevice(h->device));
    const int D = h->p.dim_d;
    if (broadcast < 0 || broadcast > 2) return fail(HC_ERR_ARG, "hc_set_state: broadcast must be 0, 1 or 2");
    if (broadcast == 2 && h->n_members % h->n_points != 0)
        return fail(HC_ERR_ARG, "%lld members do not divide into %d parameter points", (long long)h->n_members, h->n_points);
    const size_t n = (size_t)h->n_members * D;
    const size_t n_in = broadcast == 1 ? (size_t)D : (broadcast == 2 ? (size_t)h->n_points * D : n);
    for (size_t i = 0; i < n_in; i++)
        if (!std::isfinite(psi[i])) return fail(HC_ERR_ARG, "state entry %zu is not finite", i);
    if (broadcast) {
        if (h->scratch_d.ensure(n_in)) return HC_ERR_DEVICE;
        HIP_TRY(hipMemcpyAsync(h->scratch_d.p, psi, n_in * 8, hipMemcpyHostToDevice, h->stream));
        const long long per_point = broadcast == 2 ? h->n_members / h->n_points : h->n_members;
        hipLaunchKernelGGL(broadcast_state, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                           h->scratch_d.p, h->psi.p, D, (long long)h->n_members, per_point);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));
    } else {
        HIP_TRY(hipMemcpy(h->psi.p, psi, n * 8, hipMemcpyHostToDevice));
    }
    return HC_OK;
}

int hc_get_state(hc_handle *h, double *psi, int64_t first, int64_t count)
{
    if (!h || !psi || first < 0 || count < 0 || first + count > h->n_members)
        return fail(HC_ERR_ARG, "hc_get_state: bad range");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int D = h->p.dim_d;
    HIP_TRY(hipMemcpy(psi, h->psi.p + (size_t)first * D, (size_t)count * D * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_noise_host(hc_handle *h, const double *base)
{
    if (!h || !base) return fail(HC_ERR_ARG, "hc_set_noise_host: bad argument");
    if (h->n_members <= 0) return fail(HC_ERR_ARG, "hc_set_members must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    assimilation_off(h);
    const size_t n = (size_t)h->n_members * h->p.dim_d;
    if (h->base.ensure(n)) return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpy(h->base.p, base, n * 8, hipMemcpyHostToDevice));
    h->philox = false;
    h->have_noise = true;
    return HC_OK;
}

int hc_get_noise_base(hc_handle *h, double *base, int64_t first, int64_t count)
{
    if (!h || !base || h->philox || !h->base.p || first < 0 || count < 0 || first + count > h->n_members)
        return fail(HC_ERR_ARG, "hc_get_noise_base: bad argument (host noise mode only)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int D = h->p.dim_d;
    HIP_TRY(hipMemcpy(base, h->base.p + (size_t)first * D, (size_t)count * D * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_noise_philox(hc_handle *h, uint64_t seed, int64_t member_offset)
{
    if (!h || member_offset < 0) return fail(HC_ERR_ARG, "hc_set_noise_philox: bad argument");
    if (h->n_members <= 0) return fail(HC_ERR_ARG, "hc_set_members must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    assimilation_off(h);
    hipLaunchKernelGGL(fill_d, dim3((unsigned)((h->n_members + 255) / 256)), dim3(256), 0, h->stream, h->nscale.p,
                       1.0, (size_t)h->n_members);
    HIP_TRY(hipGetLastError());
    h->seed = seed;
    h->member_offset = member_offset;
    h->philox = true;
    h->have_noise = true;
    return HC_OK;
}

int hc_philox_normals(hc_handle *h, int64_t member, int64_t draw, double *out)
{
    if (!h || !out || member < 0 || draw < 0) return fail(HC_ERR_ARG, "hc_philox_normals: bad argument");
    if (!h->have_column) return fail(HC_ERR_ARG, "hc_set_column must come first");
    HIP_TRY(hipSetDevice(h->device));
    const int D = h->p.dim_d;
    if (h->scratch_d.ensure(D)) return HC_ERR_DEVICE;
    hipLaunchKernelGGL(philox_dump, dim3((D + 63) / 64), dim3(64), 0, h->stream, (unsigned long long)h->seed,
                       (long long)member, (unsigned)draw, D, h->scratch_d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->scratch_d.p, (size_t)D * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

// ---- correlated noise fields (include/hydrocol.h)
int hc_set_noise_correlation(hc_handle *h, const double *a, const double *b)
{
    if (!h || (a && !b)) return fail(HC_ERR_ARG, "hc_set_noise_correlation: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    noise_corr_off(h);                            // (and off it stays when the tables are refused)
    if (!a) return HC_OK;
    if (!h->have_noise || !h->philox)
        return fail(HC_ERR_ARG, "hc_set_noise_correlation: needs a Philox run (hc_set_noise_philox first); a host-noise "
                                "caller shapes its own vectors");
    if (h->filt_stride > 0 || h->enkf_nz)
        return fail(HC_ERR_ARG, "hc_set_noise_correlation: the %s is on and its base vectors carry history: set the "
                                "correlation first", h->filt_stride > 0 ? "particle filter" : "EnKF's noise field");
    StepArgs A;
    if (int rc = fill_args(h, A)) return rc;     // column, forcing, members and noise are in place; point keys uploaded
    const int D = h->p.dim_d, NP = h->n_points;
    const size_t n = (size_t)NP * D;
    for (size_t k = 0; k < n; k++) {
        const int p = (int)(k / D), i = (int)(k % D);
        const double ai = a[k], bi = b[k];
        if (!std::isfinite(ai) || !std::isfinite(bi))
            return fail(HC_ERR_ARG, "hc_set_noise_correlation: point %d node %d: a = %g, b = %g not finite", p, i, ai, bi);
        if (!(ai >= 0.0 && ai < 1.0) || !(bi > 0.0))
            return fail(HC_ERR_ARG, "hc_set_noise_correlation: point %d node %d: a = %g outside [0, 1) or b = %g <= 0", p, i, ai, bi);
        if (i == 0 && ai != 0.0)
            return fail(HC_ERR_ARG, "hc_set_noise_correlation: point %d: a_0 = %g, the recursion starts at node 0 (a_0 = 0)", p, ai);
        if (ai == 0.0 ? bi != 1.0 : std::fabs(ai * ai + bi * bi - 1.0) > 1e-12)
            return fail(HC_ERR_ARG, "hc_set_noise_correlation: point %d node %d: a = %g, b = %g is no unit-variance step "
                                    "(a^2 + b^2 = 1; b = 1 at a break)", p, i, ai, bi);
    }
    h->ncorr_ab.assign(a, a + n);
    h->ncorr_ab.insert(h->ncorr_ab.end(), b, b + n);
    int rc = h->ncorr_dev.ensure(2 * n);
    if (rc == HC_OK) rc = h->base.ensure((size_t)h->n_members * D);
    if (rc == HC_OK) {
        // the base vectors: the correlated draw 0 times the scales as they stand (one rounding), from here on carried
        // like the caller's -- damped in place -- and kept by a filter or a noise field set afterwards
        h->ncorr = true;
        hipError_t e = hipMemcpy(h->ncorr_dev.p, h->ncorr_ab.data(), 2 * n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess && (rc = launch_noise_fill(h, h->base.p, 1, nullptr, h->nscale.p)) == HC_OK) e = hipGetLastError();
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        if (rc == HC_OK && (e != hipSuccess || e2 != hipSuccess))
            rc = fail(HC_ERR_DEVICE, "hc_set_noise_correlation: base vectors: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    if (rc != HC_OK) noise_corr_off(h);          // refused: off
    return rc;
}

int hc_get_noise_correlation(hc_handle *h, int32_t *on, double *a, double *b)
{
    if (!h || !on) return fail(HC_ERR_ARG, "hc_get_noise_correlation: bad argument");
    *on = h->ncorr ? 1 : 0;
    if (!h->ncorr) return HC_OK;
    const size_t n = h->ncorr_ab.size() / 2;
    if (a) std::copy(h->ncorr_ab.begin(), h->ncorr_ab.begin() + n, a);
    if (b) std::copy(h->ncorr_ab.begin() + n, h->ncorr_ab.end(), b);
    return HC_OK;
}

int hc_noise_field_normals(hc_handle *h, int64_t member, int64_t draw, double *out)
{
    if (!h || !out || member < 0 || draw < 0) return fail(HC_ERR_ARG, "hc_noise_field_normals: bad argument");
    if (!h->ncorr) return hc_philox_normals(h, member, draw, out);
    HIP_TRY(hipSetDevice(h->device));
    // the point whose members' keys hold `member` (one point: its table serves every key)
    const int D = h->p.dim_d, NP = h->n_points;
    const long long mpp = h->n_members / NP;
    int point = 0;
    if (NP > 1) {
        point = -1;
        for (int k = 0; k < NP && point < 0; k++) {
            const long long first = (int)h->base_host.size() == NP ? h->base_host[(size_t)k] : h->member_offset + k * mpp;
            if (member >= first && member < first + mpp) point = k;
        }
        if (point < 0)
            return fail(HC_ERR_ARG, "hc_noise_field_normals: member %lld is no key of this handle's points", (long long)member);
    }
    // the fill kernel itself on one member: rows = {0}, draw_idx = {draw}
    const long long row0 = 0;
    const int draw32 = (int)(unsigned)draw;
    if (h->scratch_d.ensure((size_t)D + 2)) return HC_ERR_DEVICE;
    long long *rows = reinterpret_cast<long long *>(h->scratch_d.p + D);
    int *didx = reinterpret_cast<int *>(h->scratch_d.p + D + 1);
    HIP_TRY(hipMemcpyAsync(rows, &row0, 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(didx, &draw32, 4, hipMemcpyHostToDevice, h->stream));
    const double *ab = h->ncorr_dev.p;
    hipLaunchKernelGGL(noise_field_fill_kernel, dim3(1), dim3(NF_THREADS), 0, h->stream, h->scratch_d.p, 1ll, rows, didx,
                       (unsigned long long)h->seed, (long long)member, nullptr, 1ll, 1ll, D, nullptr,
                       ab + (size_t)point * D, ab + ((size_t)NP + point) * D);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->scratch_d.p, (size_t)D * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_noise_field_base(hc_handle *h, double *base, int64_t first, int64_t count)
{
    if (!h || !base || first < 0 || count < 0 || first + count > h->n_members || !(h->ncorr && h->philox))
        return fail(HC_ERR_ARG, "hc_get_noise_field_base: bad argument (a Philox run with a noise correlation set)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int D = h->p.dim_d;
    HIP_TRY(hipMemcpy(base, h->base.p + (size_t)first * D, (size_t)count * D * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_noise_field_base(hc_handle *h, const double *base)
{
    if (!h || !base || !(h->ncorr && h->philox))
        return fail(HC_ERR_ARG, "hc_set_noise_field_base: bad argument (a Philox run with a noise correlation set)");
    const size_t n = (size_t)h->n_members * h->p.dim_d;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(base[i])) return fail(HC_ERR_ARG, "hc_set_noise_field_base: entry %zu is not finite", i);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->base.p, base, n * 8, hipMemcpyHostToDevice));
    return HC_OK;
}

// One simulated day per launch for very large ensembles; smaller ones get proportionally longer launches, so that a launch
// holds ~1 M member-days of work (in-kernel noise; round 5: 64 k before) and the tail behind its slowest wavefront stays
// small: 4 096 members x D = 200 over the year 308.5 k column-days/s at 16 days per launch, 319 k at 64, 324 k at 128, 327 k at
// 364; 65 536 members 324 k at 1 day, 331 k at 4, 334 k at 16; 16 384 members 286 k at 4 days, 292 k at 64
// (gpurun_out/r5zd).  With the caller's noise every refreshed row of a launch stages members x D doubles on the device:
// there the launches stay at ~64 k member-days (include/hydrocol.h).
static int auto_rows_per_launch(int64_t n_members, bool in_kernel_noise)
{
    const int64_t target = in_kernel_noise ? (int64_t(1) << 20) : 65536;
    const int64_t days = std::max<int64_t>(1, std::min<int64_t>(target / std::max<int64_t>(n_members, 1), 365));
    return (int)(48 * days);
}

}  // extern "C"

namespace {
// staging of a launch with profile statistics: transpiration / lateral flow of every row (at most 1 GiB) and, for short
// strides, the end-of-row states of every row; about 4 GiB at most, a launch stages at least one row whatever the size
constexpr int64_t PROF_STAGE_BYTES = int64_t(4) << 30, PROF_DIAG_BYTES = int64_t(1) << 30;
constexpr long long PROF_MEMBERS_PER_BLOCK = 1024;

int launch_profile(hc_handle *h, const StepArgs &A, const ProfLayout &L, const double *stage, int64_t row, int snapshot)
{
    const long long mpp = h->n_members / h->n_points;
    const dim3 grid((unsigned)((h->p.dim_d + PROF_TILE - 1) / PROF_TILE),
                    (unsigned)((mpp + PROF_MEMBERS_PER_BLOCK - 1) / PROF_MEMBERS_PER_BLOCK), (unsigned)h->n_points);
    long long *t = h->prof.buf.p;
    hipLaunchKernelGGL(profile_kernel, grid, dim3(PROF_TILE * PROF_WAVES), 0, h->stream, A, h->node_tabs.p,
                       (int)h->use_special(), stage, h->wtd_obs.p, (long long)row, (long long)(row / h->prof_stride),
                       (long long)L.n_prow, snapshot, PROF_MEMBERS_PER_BLOCK, t + L.prof, t + L.pcnt,
                       reinterpret_cast<unsigned long long *>(t + L.ovf));
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// the soil-moisture histogram of the same row, from the same states, on the same grid
int launch_theta_hist(hc_handle *h, const StepArgs &A, const ProfLayout &L, const double *stage, int64_t row, int snapshot)
{
    const long long mpp = h->n_members / h->n_points;
    const dim3 grid((unsigned)((h->p.dim_d + PROF_TILE - 1) / PROF_TILE),
                    (unsigned)((mpp + PROF_MEMBERS_PER_BLOCK - 1) / PROF_MEMBERS_PER_BLOCK), (unsigned)h->n_points);
    const int B = h->thist_bins;
    int *t = h->thist.buf.p;
    hipLaunchKernelGGL(theta_hist_kernel, grid, dim3(PROF_TILE * PROF_WAVES), (size_t)B * PROF_TILE * sizeof(unsigned),
                       h->stream, A, h->node_tabs.p, (int)h->use_special(), stage, h->wtd_obs.p, (long long)row,
                       (long long)(row / h->prof_stride), (long long)L.n_prow, snapshot, PROF_MEMBERS_PER_BLOCK, B, t,
                       reinterpret_cast<unsigned long long *>(t + (h->thist.n - 2)));
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// the theta covariance of the same row, from the same states.  The members' quantised rows Q [P][cap][E64] uint32 are
// staged in at most COV_Q_BYTES (1 GiB: 262 144 members x E64 = 320 take 320 MiB), allocated by the first launch; a larger
// ensemble runs in chunks of `cap` members a point (a multiple of 64 unless HYDROCOL_COV_CHUNK_MEMBERS says otherwise),
// quantise then multiply, which changes no bit: every add is an integer's.  A quantise block takes 256 members (64 a wave:
// E atomics a block); a product block a slice of 4096 (a 262 144-member point at E = 302: 15 tile pairs x 64 slices).
constexpr int64_t COV_Q_BYTES = int64_t(1) << 30;
constexpr long long COV_QUANT_MEMBERS_PER_BLOCK = 256, COV_SLICE_MEMBERS = 4096;
int launch_theta_cov(hc_handle *h, const StepArgs &A, const ProfLayout &L, const double *stage, int64_t row, int snapshot)
{
    const CovLayout C = cov_layout(h);
    const long long mpp = h->n_members / h->n_points;
    long long cap = h->cov_chunk > 0
        ? h->cov_chunk
        : std::max<long long>(COV_TILE, COV_Q_BYTES / ((int64_t)h->n_points * C.E64 * 4) / COV_TILE * COV_TILE);
    cap = std::min(cap, mpp);
    if (h->cov_q.ensure((size_t)h->n_points * cap * C.E64)) return HC_ERR_DEVICE;
    long long *t = h->cov.buf.p;
    const int nt = C.E64 / COV_TILE;
    const long long prow = row / h->prof_stride;
    for (long long c0 = 0; c0 < mpp; c0 += cap) {
        const long long len = std::min(cap, mpp - c0);
        hipLaunchKernelGGL(theta_cov_quantise_kernel,
                           dim3(1, (unsigned)((len + COV_QUANT_MEMBERS_PER_BLOCK - 1) / COV_QUANT_MEMBERS_PER_BLOCK),
                                (unsigned)h->n_points),
                           dim3(PROF_TILE * PROF_WAVES), (size_t)h->p.dim_d * sizeof(double), h->stream, A, h->node_tabs.p,
                           (int)h->use_special(), stage, h->wtd_obs.p, (long long)row, prow, (long long)L.n_prow, snapshot,
                           COV_QUANT_MEMBERS_PER_BLOCK, c0, c0 + len, cap, C.s, C.n, C.E64, (long long)C.W, h->cov_q.p, t,
                           reinterpret_cast<unsigned long long *>(t + (h->cov.n - 1)));
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(theta_cov_syrk_kernel,
                           dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)((len + COV_SLICE_MEMBERS - 1) / COV_SLICE_MEMBERS),
                                (unsigned)h->n_points),
                           dim3(COV_THREADS), 0, h->stream, h->wtd_obs.p, (long long)row, prow, (long long)L.n_prow, snapshot,
                           len, cap, COV_SLICE_MEMBERS, C.E, C.E64, (long long)C.W, h->cov_q.p, t);
        HIP_TRY(hipGetLastError());
    }
    return HC_OK;
}

// the layer storage of the same row, from the same states: a block per slice of STOR_MEMBERS_PER_BLOCK members (a wave
// reads whole rows, so the slices are short: 32 members a wave make the block's set-up negligible and give a
// 262 144-member point 2048 blocks); beyond stor_grid_y = 65 535 slices (8.4 M members a point) a block takes several, so
// that grid y stays within what the runtime launches and a block's uint32 LDS counters within 2^31 / 65 535 members
constexpr long long STOR_MEMBERS_PER_BLOCK = 128;
int launch_layer_storage(hc_handle *h, const StepArgs &A, const ProfLayout &L, const double *stage, int64_t row, int snapshot)
{
    const long long mpp = h->n_members / h->n_points;
    const dim3 grid(1, (unsigned)std::min((mpp + STOR_MEMBERS_PER_BLOCK - 1) / STOR_MEMBERS_PER_BLOCK, h->stor_grid_y),
                    (unsigned)h->n_points);
    StorLayers Ly{};
    Ly.n = h->stor_layers, Ly.lo = h->p.dim_d, Ly.hi = 0;
    for (int l = 0; l < Ly.n; l++) {
        Ly.i0[l] = h->stor_range[l][0], Ly.i1[l] = h->stor_range[l][1];
        Ly.lo = std::min(Ly.lo, Ly.i0[l]), Ly.hi = std::max(Ly.hi, Ly.i1[l]);
    }
    const StorLayout S = stor_layout(h);
    const int B = h->stor_bins;
    long long *t = h->stor.buf.p;
    int *hist = B > 0 ? h->shist.buf.p : nullptr;
    const size_t lds = (size_t)h->p.dim_d * sizeof(double) + (size_t)Ly.n * B * sizeof(unsigned);
    hipLaunchKernelGGL(layer_storage_kernel, grid, dim3(PROF_TILE * PROF_WAVES), lds, h->stream, A, h->node_tabs.p,
                       (int)h->use_special(), stage, h->wtd_obs.p, (long long)row, (long long)(row / h->prof_stride),
                       (long long)L.n_prow, snapshot, STOR_MEMBERS_PER_BLOCK, Ly, B, t, t + S.scnt,
                       reinterpret_cast<unsigned long long *>(t + S.ovf), hist,
                       reinterpret_cast<unsigned long long *>(B > 0 ? hist + S.bins : nullptr));
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// The conductivities of the same row, from the same states and the row's noise vector as its solve left it
// (include/hydrocol.h): a non-refresh row -- a snapshot, row 0 -- reads the members' base, a refresh row its own vector
// damped once per failed attempt (`stats`: the row's [N][6] of the launch, NULL: none failed).  Vectors in memory when the
// step kernel reads them there (caller noise, or a Philox run whose handle fills it), else Philox as the step kernel keys
// it.  `eval` (hc_conductivity_eval): the members' values [4][N][D] instead of the table.
int launch_conductivity(hc_handle *h, const StepArgs &A, const ProfLayout &L, const double *stage, int64_t row, int snapshot,
                        const int *stats, double *eval)
{
    const int64_t N = h->n_members, D = h->p.dim_d;
    const long long mpp = N / h->n_points;
    const bool refresh = !snapshot && row > 0 && h->h_refresh[(size_t)row];
    CondNoise Z{};
    Z.stats = refresh ? stats : nullptr;
    if (A.host_noise) {
        Z.mode = refresh ? 1 : 0;
        if (refresh && h->cond_fresh_last < 0)
            return fail(HC_ERR_ARG, "conductivity statistics: row %lld refreshes the noise and no launch has staged its vector",
                        (long long)row);
        Z.vec = refresh ? h->fresh.p + (size_t)h->cond_fresh_last * N * D : h->base.p;
    } else {
        Z.mode = refresh ? 3 : 2;
        Z.nscale = h->nscale.p;
        Z.seed = h->seed;
        Z.member_offset = h->member_offset;
        Z.point_base = h->n_points > 1 ? h->point_base.p : nullptr;
        Z.draw_idx = h->draw_idx.p;
        Z.row = row;
    }
    const CondLayout C = eval ? CondLayout{} : cond_layout(h);     // (the hook touches no table: the row needs no slot)
    long long *t = eval ? nullptr : h->cond.buf.p;
    const long long prow = eval ? 0 : row / h->prof_stride;
    const dim3 grid((unsigned)((D + PROF_TILE - 1) / PROF_TILE),
                    (unsigned)((mpp + PROF_MEMBERS_PER_BLOCK - 1) / PROF_MEMBERS_PER_BLOCK), (unsigned)h->n_points);
    hipLaunchKernelGGL(conductivity_kernel, grid, dim3(PROF_TILE * PROF_WAVES), 0, h->stream, A, h->node_tabs.p,
                       (int)h->use_special(), stage, h->wtd_obs.p, (long long)row, prow, (long long)L.n_prow, snapshot,
                       PROF_MEMBERS_PER_BLOCK, Z, t, eval ? nullptr : t + C.kcnt,
                       reinterpret_cast<unsigned long long *>(eval ? nullptr : t + C.ovf), eval);
    HIP_TRY(hipGetLastError());
    if (eval || h->cond_layers <= 0) return HC_OK;
    StorLayers Ly{};
    Ly.n = h->cond_layers, Ly.lo = (int)D, Ly.hi = 0;
    for (int l = 0; l < Ly.n; l++) {
        Ly.i0[l] = h->cond_range[l][0], Ly.i1[l] = h->cond_range[l][1];
        Ly.lo = std::min(Ly.lo, Ly.i0[l]), Ly.hi = std::max(Ly.hi, Ly.i1[l]);
    }
    const dim3 lgrid(1, (unsigned)std::min((mpp + STOR_MEMBERS_PER_BLOCK - 1) / STOR_MEMBERS_PER_BLOCK, h->stor_grid_y),
                     (unsigned)h->n_points);
    hipLaunchKernelGGL(conductivity_layer_kernel, lgrid, dim3(PROF_TILE * PROF_WAVES), (size_t)3 * D * sizeof(double),
                       h->stream, A, h->node_tabs.p, (int)h->use_special(), stage, h->wtd_obs.p, (long long)row, prow,
                       (long long)L.n_prow, snapshot, STOR_MEMBERS_PER_BLOCK, Ly, Z, t + C.kmom_layer, t + C.kcnt_layer,
                       reinterpret_cast<unsigned long long *>(t + C.ovf));
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// the period (index into per_end) that forcing row `row` belongs to, -1: after the last end
int64_t period_of(const hc_handle *h, int64_t row)
{
    const auto it = std::lower_bound(h->per_end.begin(), h->per_end.end(), row);
    return it == h->per_end.end() ? -1 : (int64_t)(it - h->per_end.begin());
}

// The root uptake (hc_set_root_uptake) of the launch's daylight rows from their staged end states, added to the members'
// accumulators and to the period's depth profile: layer_storage_kernel's slices (a wave reads whole rows: 32 members a
// wave, 2048 blocks for a 262 144-member point; grid y capped as there).  A night row has no uptake and launches
// nothing; a skipped row returns at the kernel's first line.  theta_out / u_out: the test hook's launch on the current
// states (stage = psi) of row `row0`, night rows included.
constexpr long long UPT_MEMBERS_PER_BLOCK = 128;
size_t uptake_lds_bytes(const hc_handle *h, bool eval)
{
    int n_int = 0;
    for (const ColumnDev &P : h->P_host) n_int = std::max(n_int, P.n_root_int);
    const int n_model = eval ? h->p.dim_d - 1 : n_int + 1;
    const size_t cells = (size_t)((n_model + PROF_TILE - 1) / PROF_TILE) * PROF_TILE;
    return ((UPT_NTAB + PROF_WAVES) * cells + 2 * (size_t)(n_int + 1)) * sizeof(double);
}
int launch_root_uptake(hc_handle *h, const StepArgs &A, const double *stage, int64_t row0, int rows, double *theta_out,
                       double *u_out)
{
    const bool eval = theta_out != nullptr;
    const int64_t N = h->n_members, D = h->p.dim_d;
    const long long mpp = N / h->n_points;
    const dim3 grid(1, (unsigned)std::min((mpp + UPT_MEMBERS_PER_BLOCK - 1) / UPT_MEMBERS_PER_BLOCK, h->stor_grid_y),
                    (unsigned)h->n_points);
    UptLayers Ly{};
    Ly.n = eval ? 0 : h->upt_layers;
    for (int l = 0; l < Ly.n; l++) Ly.c0[l] = h->upt_range[l][0], Ly.c1[l] = h->upt_range[l][1];
    const size_t lds = uptake_lds_bytes(h, eval);
    if (eval) {
        hipLaunchKernelGGL(root_uptake_kernel, grid, dim3(PROF_TILE * PROF_WAVES), lds, h->stream, A, h->mid_tabs.p,
                           (int)h->use_special(), stage, h->wtd_obs.p, h->atm.p, h->daylight.p, (long long)row0, 0LL, 1LL,
                           UPT_MEMBERS_PER_BLOCK, Ly, nullptr, nullptr, nullptr, theta_out, u_out);
        HIP_TRY(hipGetLastError());
        return HC_OK;
    }
    const int64_t p = period_of(h, row0);
    if (p < 0) return HC_OK;
    const UptLayout U = uptake_layout(h);
    long long *t = h->upt.buf.p;
    const int n = (int)std::min<int64_t>(rows, h->per_end[(size_t)p] - row0 + 1);
    for (int r = 0; r < n; r++) {
        const int64_t row = row0 + r;
        if (!(h->h_daylight[(size_t)row] & 1) || h->h_wtd_obs[(size_t)row] < 0) continue;
        hipLaunchKernelGGL(root_uptake_kernel, grid, dim3(PROF_TILE * PROF_WAVES), lds, h->stream, A, h->mid_tabs.p,
                           (int)h->use_special(), stage + (size_t)r * N * D, h->wtd_obs.p, h->atm.p, h->daylight.p,
                           (long long)row, (long long)p, (long long)h->per_n, UPT_MEMBERS_PER_BLOCK, Ly, h->uacc.buf.p,
                           t + U.uprof, reinterpret_cast<unsigned long long *>(t + U.ovf), nullptr, nullptr);
        HIP_TRY(hipGetLastError());
    }
    return HC_OK;
}

// the end of period p for the uptake: before period_reduce_kernel, whose `wtd_shallowest` plane says who is counted
constexpr long long PERIOD_MEMBERS_PER_BLOCK = 1024;
int launch_uptake_reduce(hc_handle *h, int64_t p)
{
    const int64_t N = h->n_members;
    const long long mpp = N / h->n_points;
    const UptLayout U = uptake_layout(h);
    const int B = h->upt_bins, L = h->upt_layers;
    long long *t = h->upt.buf.p;
    int *hist = B > 0 ? h->uhist.buf.p : nullptr;
    const dim3 grid((unsigned)((mpp + PERIOD_MEMBERS_PER_BLOCK - 1) / PERIOD_MEMBERS_PER_BLOCK), (unsigned)h->n_points);
    hipLaunchKernelGGL(uptake_reduce_kernel, grid, dim3(PERIOD_THREADS), (size_t)L * B * sizeof(unsigned), h->stream,
                       h->uacc.buf.p, h->pacc.buf.p + 2 * N, (long long)N, mpp, PERIOD_MEMBERS_PER_BLOCK, (long long)p,
                       (long long)h->per_n, L, B, t, t + U.ucnt, reinterpret_cast<unsigned long long *>(t + U.ovf), hist,
                       reinterpret_cast<unsigned long long *>(B > 0 ? hist + U.bins : nullptr));
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// The launch's rows [row0, row0 + rows) added to the members' accumulators (plan_chunk ended the launch on the period's
// end row at the latest, so they lie in one period) and, when the launch ends on the end row, the period reduced over
// the members of each point: slices of PERIOD_MEMBERS_PER_BLOCK members (four a thread) give a 262 144-member point
// 256 blocks, one a CU.  The root uptake (hc_set_root_uptake), whose rows the caller has added already, is reduced first:
// it counts the members this reduction is about to count and reset.
int launch_period(hc_handle *h, int64_t row0, int rows)
{
    const int64_t p = period_of(h, row0);
    if (p < 0) return HC_OK;
    const int64_t end_row = h->per_end[(size_t)p], N = h->n_members;
    const PeriodLayout L = period_layout(h);
    long long *t = h->pmom.buf.p;
    unsigned long long *ovf = reinterpret_cast<unsigned long long *>(t + L.ovf);
    PeriodThresholds Th{};
    Th.n = h->per_nthr;
    for (int j = 0; j < Th.n; j++) Th.node[j] = h->per_thr[j];
    const int n = (int)std::min<int64_t>(rows, end_row - row0 + 1);
    hipLaunchKernelGGL(period_accumulate_kernel, dim3((unsigned)((N + PERIOD_THREADS - 1) / PERIOD_THREADS)),
                       dim3(PERIOD_THREADS), 0, h->stream, h->diag.p, h->wtd_u16.p, h->wtd_obs.p, (long long)N,
                       (long long)row0, n, Th, h->pacc.buf.p, ovf);
    HIP_TRY(hipGetLastError());
    if (row0 + rows - 1 < end_row) return HC_OK;
    if (h->upt_layers > 0)
        if (int rc = launch_uptake_reduce(h, p)) return rc;
    const long long mpp = N / h->n_points;
    const int B = h->per_bins, D = (int)h->p.dim_d;
    int *hist = B > 0 ? h->phist.buf.p : nullptr;
    const dim3 grid((unsigned)((mpp + PERIOD_MEMBERS_PER_BLOCK - 1) / PERIOD_MEMBERS_PER_BLOCK), (unsigned)h->n_points);
    const size_t lds = B > 0 ? (size_t)2 * (B + D) * sizeof(unsigned) : 0;
    hipLaunchKernelGGL(period_reduce_kernel, grid, dim3(PERIOD_THREADS), lds, h->stream, h->pacc.buf.p, (long long)N, mpp,
                       PERIOD_MEMBERS_PER_BLOCK, (long long)p, (long long)h->per_n, L.K, B, D, 20 + h->per_fexp[0],
                       20 + h->per_fexp[1], t, t + L.pcnt, ovf, hist, B > 0 ? hist + L.wtd : nullptr,
                       reinterpret_cast<unsigned long long *>(B > 0 ? hist + L.entries : nullptr));
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

constexpr long long HIST_MEMBERS_PER_BLOCK = 4096;

// the histogram rows among launch rows [row0, row0 + chunk) of the water-table indices in wtd_u16
int launch_hist(hc_handle *h, int64_t row0, int chunk)
{
    const int64_t s = h->hist_stride;
    const int64_t first = (s - row0 % s) % s;
    if (first >= chunk) return HC_OK;
    const int64_t n_here = (chunk - 1 - first) / s + 1;
    const long long mpp = h->n_members / h->n_points;
    // at most 65536 slices per row keeps the grid's x extent (rows x slices) far below 2^31
    const long long mpb = std::max(HIST_MEMBERS_PER_BLOCK, (mpp + 65535) / 65536);
    const long long slices = (mpp + mpb - 1) / mpb;
    hipLaunchKernelGGL(wtd_hist_kernel, dim3((unsigned)(n_here * slices), (unsigned)h->n_points), dim3(HIST_THREADS), 0,
                       h->stream, h->wtd_u16.p, h->wtd_obs.p, (long long)h->n_members, mpp, mpb, (int)slices,
                       (long long)row0, (int)first, (int)s, (long long)hist_rows(h), h->p.dim_d, h->hist.buf.p);
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

int wtd_distribution_run(const int32_t *hist, const int32_t *obs_idx, int64_t n_rows, int32_t D, const WtdLevels &lv,
                         int32_t n_levels, double dz, int64_t *count, int32_t *quantile_idx, double *crps_cm,
                         DevBuf<int> &d_hist, DevBuf<int> &d_obs, DevBuf<long long> &d_count, DevBuf<int> &d_q,
                         DevBuf<double> &d_crps)
{
    const size_t R = (size_t)n_rows;
    if (d_hist.ensure(R * D) || d_obs.ensure(R) || d_count.ensure(R) || d_q.ensure(R * std::max(n_levels, 1)) ||
        d_crps.ensure(R))
        return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpy(d_hist.p, hist, R * D * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_obs.p, obs_idx, R * 4, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 2048);
    hipLaunchKernelGGL(wtd_dist_kernel, dim3(blocks), dim3(256), 0, nullptr, d_hist.p, d_obs.p, (long long)n_rows, (int)D, lv,
                       (int)n_levels, dz, d_count.p, d_q.p, d_crps.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(count, d_count.p, R * 8, hipMemcpyDeviceToHost));
    if (n_levels > 0) HIP_TRY(hipMemcpy(quantile_idx, d_q.p, R * n_levels * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(crps_cm, d_crps.p, R * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

// ------------------------------------------------------------------ hc_step_rows, one launch at a time
// The rows of one launch and where its profile rows are read from.
struct Chunk {
    int64_t row0 = 0;             // first forcing row
    int rows = 0;
    bool stage_all = false;       // the end states of every row are staged through psi_rows
    bool end_on_profile = false;  // the launch ends ON a profile row: its states are the members' current states
};

// The launch after `done` rows of the request.  Per-row outputs are staged in device buffers of rows x members entries:
// a caller that asks for them gets shorter launches, so that the largest (psi_rows: 8 D bytes per member-row) stays
// within ~1 GiB however long the request.  Profile rows (the step kernels are not changed for them; results do not
// depend on launch length):
//  stride >= the rows the staging cap admits: the launch ends ON the next profile row, whose states are then the
//    members' current states (no staging at all);
//  shorter strides: every row of the launch is staged through psi_rows (as psi_rows_out does), the launch
//    shortened to the cap, and the profile rows are read from there.
// a filtered Philox run stages the launch's refresh vectors (N D doubles each) on the device: about 4 GiB at most
constexpr int64_t FILT_FRESH_BYTES = int64_t(4) << 30;

bool is_assimilation_row(const hc_handle *h, int64_t row)
{
    const int64_t s = assim(h).stride;
    return s > 0 && row >= 1 && row % s == 0 && h->h_wtd_obs[(size_t)row] >= 0;
}

// The offset slot that lagged row `row` fills for the assimilation row after it (hc_set_enkf_window,
// hc_set_filter_window), -1: none.  The row takes part when it is >= 1 and has an observation, and the assimilation row
// is one as things stand.
int window_slot(const hc_handle *h, int64_t row)
{
    const std::vector<int> &off = assim(h).win.off;
    const int64_t s = assim(h).stride;
    if (off.empty() || s <= 0 || row < 1 || h->h_wtd_obs[(size_t)row] < 0) return -1;
    const int64_t r = (row / s + 1) * s;
    if (r >= h->n_rows || !is_assimilation_row(h, r)) return -1;
    for (size_t j = 0; j < off.size(); j++)
        if (off[j] == r - row) return (int)j;
    return -1;
}

// The launch after `done` rows of the request.  With a filter on, a launch ends on the next assimilation row and, in a
// Philox run with the particle filter, holds at most as many refresh rows as FILT_FRESH_BYTES admits (so does any launch
// of a Philox run that stages its vectors: the noise field's, a correlated source's); with either filter's window on it
// ends on the next lagged row that takes part.
Chunk plan_chunk(const hc_handle *h, const hc_step_args *a, int64_t done, bool prof_on)
{
    const int64_t N = h->n_members, D = h->p.dim_d;
    int64_t out_bytes_per_row = 0;
    if (a->psi_rows_out) out_bytes_per_row += N * D * 8;
    if (a->stats_out) out_bytes_per_row += N * 6 * 4;
    if (a->diag_out) out_bytes_per_row += N * 2 * 8;
    if (a->wtd_out) out_bytes_per_row += N * 4;
    const int64_t rows_cap = out_bytes_per_row > 0 ? std::max<int64_t>(1, (int64_t(1) << 30) / out_bytes_per_row) : INT32_MAX;
    int per_launch = h->rows_per_launch > 0 ? h->rows_per_launch : auto_rows_per_launch(N, h->philox);
    if (h->rows_per_launch <= 0) per_launch = (int)std::min<int64_t>(per_launch, rows_cap);
    Chunk c;
    c.rows = (int)std::min<int64_t>(per_launch, a->n_rows - done);
    c.row0 = a->spinup ? a->row_begin : a->row_begin + done;
    if (const int64_t s = assim(h).stride; s > 0 && !a->spinup) {
        for (int64_t r = std::max<int64_t>(s, (c.row0 + s - 1) / s * s); r < c.row0 + c.rows; r += s)
            if (is_assimilation_row(h, r)) {
                c.rows = (int)(r - c.row0 + 1);
                break;
            }
        if (assim(h).win.n > 0)
            for (int r = 0; r < c.rows; r++)
                if (window_slot(h, c.row0 + r) >= 0) {
                    c.rows = r + 1;
                    break;
                }
    }
    if (h->noise_host() && !a->spinup) {      // (with a correlation set also without a filter)
        const int64_t cap = std::max<int64_t>(1, FILT_FRESH_BYTES / (N * D * 8));
        int64_t n_fresh = 0;
        for (int r = 0; r < c.rows; r++)
            if (h->h_refresh[(size_t)(c.row0 + r)] && ++n_fresh > cap) {
                c.rows = r;
                break;
            }
    }
    const int64_t diag_row = N * 2 * 8;
    if (h->per_n > 0 && !a->spinup) {
        // period totals (hc_set_period_totals): a launch ends on the period's end row, and diag is staged as for the profiles
        if (const int64_t p = period_of(h, c.row0); p >= 0)
            c.rows = (int)std::min<int64_t>(c.rows, h->per_end[(size_t)p] - c.row0 + 1);
        c.rows = (int)std::min<int64_t>(c.rows, std::max<int64_t>(1, PROF_DIAG_BYTES / diag_row));
    }
    // the root uptake (hc_set_root_uptake) reads every row's end state: staged as for a short profile stride
    const bool upt_on = h->upt_layers > 0 && !a->spinup;
    if (!prof_on && !upt_on) return c;
    const int64_t s = h->prof_stride, row_bytes = N * D * 8;
    c.rows = (int)std::min<int64_t>(c.rows, std::max<int64_t>(1, PROF_DIAG_BYTES / diag_row));
    const int64_t cap_rows = std::max<int64_t>(1, (PROF_STAGE_BYTES - (int64_t)c.rows * diag_row) / row_bytes);
    if (a->psi_rows_out) {
        c.stage_all = true;       // every row is staged for the caller already
    } else if (!upt_on && s >= cap_rows) {
        const int64_t next = (c.row0 + s - 1) / s * s;
        c.rows = (int)std::min<int64_t>(c.rows, next - c.row0 + 1);
        c.end_on_profile = (c.row0 + c.rows - 1) % s == 0;
    } else {
        c.rows = (int)std::min<int64_t>(c.rows, cap_rows);
        c.stage_all = true;
    }
    // the conductivity statistics (hc_set_conductivity_stats) read the base vectors and scales as the profile row left
    // them: the launch ends on it, staged or not
    if (prof_on && h->cond_on) c.rows = (int)std::min<int64_t>(c.rows, (c.row0 + s - 1) / s * s - c.row0 + 1);
    return c;
}

// the caller's noise vectors of the launch's refresh rows, on the device (host noise); n_fresh: how many
int stage_noise(hc_handle *h, const hc_step_args *a, const Chunk &c, int64_t consumed, int &n_fresh)
{
    const int64_t N = h->n_members, D = h->p.dim_d;
    n_fresh = 0;
    if (!a->spinup)
        for (int r = 0; r < c.rows; r++) n_fresh += h->h_refresh[(size_t)(c.row0 + r)] ? 1 : 0;
    if (n_fresh == 0) return HC_OK;
    if (h->noise_host()) {
        // the kernel's own normals of the launch's refresh rows, keyed by each slot's stream and the row's draw index
        h->filt_rows_host.clear();
        for (int r = 0; r < c.rows; r++)
            if (h->h_refresh[(size_t)(c.row0 + r)]) h->filt_rows_host.push_back(c.row0 + r);
        const size_t cnt = (size_t)n_fresh * N * D;
        if (h->fresh.ensure(cnt) || h->filt_rows.ensure((size_t)n_fresh)) return HC_ERR_DEVICE;
        HIP_TRY(hipMemcpyAsync(h->filt_rows.p, h->filt_rows_host.data(), (size_t)n_fresh * 8, hipMemcpyHostToDevice,
                               h->stream));
        if (int rc = launch_noise_fill(h, h->fresh.p, n_fresh, h->filt_rows.p, nullptr)) return rc;
        HIP_TRY(hipGetLastError());
        return HC_OK;
    }
    if (h->philox) return HC_OK;
    if (!a->fresh_noise) return fail(HC_ERR_ARG, "host noise mode: fresh_noise is NULL but rows refresh");
    const size_t cnt = (size_t)n_fresh * N * D;
    if (h->fresh.ensure(cnt)) return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpyAsync(h->fresh.p, a->fresh_noise + (size_t)consumed * N * D, cnt * 8, hipMemcpyHostToDevice, h->stream));
    return HC_OK;
}

// the launch's staging buffers and IoArgs, the points' walk order, and the step kernel between the two timing events
// (diag_on: the profile statistics or the period totals read the launch's diag; stats_on: the conductivity statistics read
// the failed attempts of its last row)
int launch_chunk(hc_handle *h, StepArgs &A, const hc_step_args *a, const Chunk &c, bool diag_on, bool stats_on)
{
    const int64_t N = h->n_members, D = h->p.dim_d;
    const size_t rows = (size_t)c.rows;
    if (h->wtd_u16.ensure(rows * N)) return HC_ERR_DEVICE;
    if ((a->stats_out || stats_on) && h->stats.ensure(rows * N * 6)) return HC_ERR_DEVICE;
    if (a->psi_rows_out && h->psi_rows.ensure(rows * N * D)) return HC_ERR_DEVICE;
    if ((a->diag_out || diag_on) && h->diag.ensure(rows * N * 2)) return HC_ERR_DEVICE;
    if (c.stage_all && h->psi_rows.ensure(rows * N * D)) return HC_ERR_DEVICE;
    h->io_host.fresh = h->fresh.p;
    h->io_host.row_begin = c.row0;
    A.n_rows = c.rows;
    A.spinup = a->spinup;
    h->io_host.wtd_u16 = h->wtd_u16.p;
    h->io_host.stats = (a->stats_out || stats_on) ? h->stats.p : nullptr;
    h->io_host.psi_rows = (a->psi_rows_out || c.stage_all) ? h->psi_rows.p : nullptr;
    h->io_host.diag = (a->diag_out || diag_on) ? h->diag.p : nullptr;
    h->io_host.fmul = nullptr;
    h->fp_day_next = -1;
    if (h->fp_on && !a->spinup)
        if (int rc = launch_forcing_fill(h, c.row0, c.rows)) return rc;
    if (int rc = push_io(h)) return rc;
    if (h->n_points > 1) {
        HIP_TRY(hipMemcpyAsync(h->point_order.p, h->order_host.data(), (size_t)h->n_points * 4, hipMemcpyHostToDevice,
                               h->stream));
        HIP_TRY(hipMemsetAsync(h->point_cost.p, 0, (size_t)h->n_points * 8, h->stream));
    }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    if (int rc = launch_step(h, A)) return rc;
    forcing_fill_commit(h);      // the step launch is issued: the perturbed forcing's state stands at its last day
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    return HC_OK;
}

// what the launch adds to the accumulated tables: moments, histograms, profile rows and fluxes
int accumulate(hc_handle *h, const StepArgs &A, const hc_step_args *a, const Chunk &c, bool prof_on, bool hist_on)
{
    const int64_t N = h->n_members, D = h->p.dim_d;
    if (a->accumulate_moments) {
        hipLaunchKernelGGL(moments_kernel, dim3(c.rows, h->n_points), dim3(256), 0, h->stream, h->wtd_u16.p,
                           h->wtd_obs.p, (long long)N, (long long)(N / h->n_points), (long long)c.row0,
                           (long long)h->n_rows, h->moments.buf.p);
        HIP_TRY(hipGetLastError());
    }
    if (hist_on)
        if (int rc = launch_hist(h, c.row0, c.rows)) return rc;
    if (h->upt_layers > 0 && !a->spinup) {
        if (!c.stage_all) return fail(HC_ERR_DEVICE, "root uptake: the launch's rows are not staged (internal error)");
        if (int rc = launch_root_uptake(h, A, h->psi_rows.p, c.row0, c.rows, nullptr, nullptr)) return rc;
    }
    if (h->per_n > 0 && !a->spinup)
        if (int rc = launch_period(h, c.row0, c.rows)) return rc;
    if (!prof_on) return HC_OK;
    const ProfLayout PL = prof_layout(h);
    for (int r = 0; r < c.rows; r++) {
        if ((c.row0 + r) % h->prof_stride != 0) continue;
        const double *stage = c.stage_all ? h->psi_rows.p + (size_t)r * N * D : h->psi.p;
        if (!c.stage_all && !(c.end_on_profile && r == c.rows - 1))
            return fail(HC_ERR_DEVICE, "profile row %lld not staged (internal error)", (long long)(c.row0 + r));
        if (int rc = launch_profile(h, A, PL, stage, c.row0 + r, 0)) return rc;
        if (h->thist_bins > 0)
            if (int rc = launch_theta_hist(h, A, PL, stage, c.row0 + r, 0)) return rc;
        if (h->stor_layers > 0)
            if (int rc = launch_layer_storage(h, A, PL, stage, c.row0 + r, 0)) return rc;
        if (h->cov_stride > 0)
            if (int rc = launch_theta_cov(h, A, PL, stage, c.row0 + r, 0)) return rc;
        if (h->cond_on) {
            if (r != c.rows - 1) return fail(HC_ERR_DEVICE, "profile row %lld does not end its launch (internal error)",
                                             (long long)(c.row0 + r));
            if (int rc = launch_conductivity(h, A, PL, stage, c.row0 + r, 0, h->stats.p + (size_t)r * N * 6, nullptr)) return rc;
        }
    }
    long long *t = h->prof.buf.p;
    hipLaunchKernelGGL(flux_stats_kernel, dim3(c.rows, h->n_points), dim3(256), 0, h->stream, h->diag.p, h->wtd_u16.p,
                       h->wtd_obs.p, (long long)N, (long long)(N / h->n_points), (long long)c.row0,
                       (long long)h->n_rows, t + PL.flux, t + PL.fcnt, t + PL.aerr,
                       reinterpret_cast<unsigned long long *>(t + PL.ovf));
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// the per-row outputs the caller asked for: rows [done, done + c.rows) of its arrays
int copy_outputs(hc_handle *h, hc_step_args *a, const Chunk &c, int64_t done)
{
    const int64_t N = h->n_members, D = h->p.dim_d;
    const size_t rows = (size_t)c.rows;
    if (a->wtd_out) {
        const size_t cnt = rows * N;
        if (h->scratch_i.ensure(cnt)) return HC_ERR_DEVICE;
        hipLaunchKernelGGL(widen_u16, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, h->wtd_u16.p,
                           h->scratch_i.p, cnt);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(a->wtd_out + (size_t)done * N, h->scratch_i.p, cnt * 4, hipMemcpyDeviceToHost, h->stream));
    }
    if (a->stats_out)
        HIP_TRY(hipMemcpyAsync(a->stats_out + (size_t)done * N * 6, h->stats.p, rows * N * 6 * 4, hipMemcpyDeviceToHost,
                               h->stream));
    if (a->psi_rows_out)
        HIP_TRY(hipMemcpyAsync(a->psi_rows_out + (size_t)done * N * D, h->psi_rows.p, rows * N * D * 8,
                               hipMemcpyDeviceToHost, h->stream));
    if (a->diag_out)
        HIP_TRY(hipMemcpyAsync(a->diag_out + (size_t)done * N * 2, h->diag.p, rows * N * 2 * 8, hipMemcpyDeviceToHost,
                               h->stream));
    return HC_OK;
}

// A callback of a sharded assimilation (hc_set_filter_shard) runs on a drained stream; one that fails fails the step.
int filter_shard_call(hc_handle *h, const char *what, int rc)
{
    if (rc) return fail(HC_ERR_DEVICE, "the filter shard's %s callback returned %d (shard %d of %d)", what, rc, h->fs_index,
                        h->fs_n);
    return HC_OK;
}

// The routing of a sharded assimilation, after the ancestry of the whole point: every slot's rank among the distinct
// ancestors, the routing table, the columns to send packed, the counts on the host, the caller's exchange, and the
// handle's slots gathered from its own members and the receive region into the second buffers.
int filter_shard_resample(hc_handle *h, int64_t n_tiles)
{
    const int64_t N = h->n_members, D = h->p.dim_d, S = h->fs_n, me = h->fs_index, np = h->fs_bounds[(size_t)S];
    const FilterShardLayout L = filter_shard_layout(np, N, S, D);
    const long long *anc = h->filt_anc.p, *bounds = h->fs_bounds_dev.p;
    long long *const send = h->fs_buf + L.send, *const recv = h->fs_buf + L.recv;
    const long long list_cap = (long long)(N + S - 1);
    hipLaunchKernelGGL(filter_shard_rank_kernel, dim3((unsigned)n_tiles), dim3(FILT_THREADS), 0, h->stream, anc, (long long)np,
                       h->filt_tiles.p, (long long *)nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_tile_scan_kernel, dim3(1), dim3(FILT_THREADS), 0, h->stream, (long long)n_tiles,
                       h->filt_tiles.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_shard_rank_kernel, dim3((unsigned)n_tiles), dim3(FILT_THREADS), 0, h->stream, anc, (long long)np,
                       h->filt_tiles.p, h->fs_rank.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_route_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, anc, h->fs_rank.p,
                       bounds, (int)S, (int)me, h->fs_table.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_tile_scan_kernel, dim3(2), dim3(FILT_THREADS), 0, h->stream, (long long)S,
                       h->fs_table.p + 2 * S);
    HIP_TRY(hipGetLastError());
    const unsigned slot_blocks = (unsigned)std::min<int64_t>((np + 255) / 256, (int64_t)h->n_cu * 64);
    hipLaunchKernelGGL(filter_route_fill_kernel, dim3(slot_blocks), dim3(256), 0, h->stream, anc, h->fs_rank.p, bounds, (int)S,
                       (int)me, h->fs_table.p, (long long)np, h->fs_list.p, list_cap, h->fs_src.p);
    HIP_TRY(hipGetLastError());
    const long long *psi = reinterpret_cast<const long long *>(h->psi.p), *base = reinterpret_cast<const long long *>(h->base.p);
    const size_t most = (size_t)list_cap * 2 * D, total = (size_t)N * D;
    hipLaunchKernelGGL(filter_pack_kernel, dim3((unsigned)std::min<size_t>((most + 255) / 256, (size_t)h->n_cu * 64)), dim3(256),
                       0, h->stream, h->fs_list.p, h->fs_table.p, (int)S, list_cap, (long long)N, psi, base, send, (int)D);
    HIP_TRY(hipGetLastError());
    h->fs_counts.resize((size_t)(2 * S));
    HIP_TRY(hipMemcpyAsync(h->fs_counts.data(), h->fs_table.p, (size_t)(2 * S) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->fs_recv_words.resize((size_t)S);
    h->fs_send_words.resize((size_t)S);
    int64_t n_recv = 0, n_send = 0;
    for (int64_t s = 0; s < S; s++) {
        n_recv += h->fs_counts[(size_t)s];
        n_send += h->fs_counts[(size_t)(S + s)];
        h->fs_recv_words[(size_t)s] = h->fs_counts[(size_t)s] * 2 * D;
        h->fs_send_words[(size_t)s] = h->fs_counts[(size_t)(S + s)] * 2 * D;
    }
    if (n_recv > N || n_send > list_cap)
        return fail(HC_ERR_DEVICE, "the filter shard's gathered water-table indices give no monotone ancestry (%lld columns "
                    "to receive, %lld to send, %lld members): the gather callback did not deliver", (long long)n_recv,
                    (long long)n_send, (long long)N);
    if (int rc = filter_shard_call(h, "routing", h->fs_route(h->fs_ctx, send, h->fs_send_words.data(), recv,
                                                             h->fs_recv_words.data())))
        return rc;
    hipLaunchKernelGGL(filter_shard_gather_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, (size_t)h->n_cu * 64)),
                       dim3(256), 0, h->stream, h->fs_src.p, psi, base, recv, reinterpret_cast<long long *>(h->psi_alt.p),
                       reinterpret_cast<long long *>(h->base_alt.p), (long long)N, (int)D);
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// one entry of the sensor table from a pass over the present sensors' theta: the squared deviations from the means on
// the device (entries 3 and 5: a std), or the sums (entry 4: the posterior mean); anc: over the resampled slots.  The
// forecast's std (entry 3) takes the lagged depths of the window along, into the window's table.
int filter_sm_moment(hc_handle *h, const EnkfRow &s, const long long *anc, int entry, int64_t n_tiles, int64_t n_arow,
                     int64_t slot)
{
    const int64_t N = h->n_members, P = h->n_points, mpp = N / P;
    const int n_cols = entry == 3 ? s.m : s.ms;
    if (n_cols == 0) return HC_OK;
    hipLaunchKernelGGL(filter_tile_partial_kernel, dim3((unsigned)n_tiles, (unsigned)P), dim3(FILT_THREADS), 0, h->stream,
                       h->filt_Y.p, s.m + 2, 1, n_cols, anc, entry == 4 ? (const double *)nullptr : h->filt_sums.p,
                       (long long)mpp, (long long)N, (long long)n_tiles, h->filt_part.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_sm_moment_kernel, dim3((unsigned)P), dim3(WAVE), 0, h->stream, h->filt_part.p,
                       (long long)n_tiles, (long long)mpp, s, n_cols, entry, (long long)n_arow, (long long)slot,
                       h->filt_sums.p, h->filt_sm.table.buf.p, h->filt_win.table.buf.p);
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// The observations of assimilation row `row` beyond the well's: the record's sensors with a value, in record order, then
// the lagged rows of the window that were captured for it, by ascending offset: well-type columns of the well's sigma,
// node = the lagged row's observed index (which only the particle filter's kernels read: the EnKF's stop at ms)
EnkfRow assim_row(const hc_handle *h, const SmRecord &r, const WindowBase &w, double well_sigma, int64_t row)
{
    EnkfRow s{};
    for (int i = 0; i < r.n; i++) {
        const double v = r.values[(size_t)row * r.n + i];
        if (std::isnan(v)) continue;
        s.sensor[s.m] = i;
        s.node[s.m] = r.nodes[(size_t)i];
        s.obs[s.m] = v;
        s.sigma[s.m] = r.sigma[(size_t)i];
        s.m++;
    }
    s.ms = s.m;
    s.n = s.ms > 0 ? r.n : 0;
    for (int j = 0; j < w.n; j++) {
        const int64_t rj = row - w.off[(size_t)j];
        if (rj < 1 || h->h_wtd_obs[(size_t)rj] < 0 || w.row[(size_t)j] != rj) continue;
        s.sensor[s.m] = j;
        s.node[s.m] = h->h_wtd_obs[(size_t)rj];
        s.obs[s.m] = h->p.dz * (double)h->h_wtd_obs[(size_t)rj];
        s.sigma[s.m] = well_sigma;
        s.wrow[s.m] = (unsigned)rj;
        s.m++;
    }
    s.nw = s.m > s.ms ? w.n : 0;
    return s;
}

// The lagged row the launch ended on (hc_set_filter_window): every member's water-table index into the window's buffer
int filter_capture(hc_handle *h, const Chunk &c, int slot)
{
    const int64_t N = h->n_members;
    if (h->filt_win.cap.ensure((size_t)(h->filt_win.n * N))) return HC_ERR_DEVICE;
    const unsigned short *w = h->wtd_u16.p + (size_t)(c.rows - 1) * N;
    hipLaunchKernelGGL(window_capture_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, w, (long long)N,
                       h->filt_win.cap.p + (size_t)slot * N);
    HIP_TRY(hipGetLastError());
    h->filt_win.row[(size_t)slot] = c.row0 + c.rows - 1;
    return HC_OK;
}

// A sensor row's weights (hc_set_filter_soil_moisture) in place of filter_weights_kernel's: theta and l_m per member, the
// tiles' maxima, e_m and q_m per member with the tiles' integer sums, the partials of (theta, e), then per point the
// diagnostics, the forecast means and the draw, and the forecast spread in a second pass about the means.  A row with
// lagged rows of the window (hc_set_filter_window) runs the same kernels with their columns between theta and e, also
// when no sensor has a value; what counts a member is then the largest of its indices (fwin_wmax).
int filter_member_weights(hc_handle *h, const Chunk &c, const EnkfRow &s, const long long *pbase, long long key)
{
    const int64_t N = h->n_members, D = h->p.dim_d, P = h->n_points, mpp = N / P;
    const int64_t row = c.row0 + c.rows - 1, slot = row / h->filt_stride, n_arow = assim_rows(h);
    const int64_t n_tiles = (mpp + FILT_TILE - 1) / FILT_TILE;
    const int width = s.m + 2;
    const bool lagged = s.m > s.ms;
    if (lagged && h->fwin_wmax.ensure((size_t)N)) return HC_ERR_DEVICE;
    if (h->filt_qm.ensure((size_t)N) || h->filt_Y.ensure((size_t)(N * (h->filt_sm.n + h->filt_win.n + 2))) ||
        h->filt_lmax.ensure((size_t)(P * n_tiles)) || h->filt_ipart.ensure((size_t)(P * n_tiles * 4)) ||
        h->filt_part.ensure((size_t)(P * n_tiles * FILT_COLS)) || h->filt_sums.ensure((size_t)(P * (FILT_COLS + 1))))
        return HC_ERR_DEVICE;
    const unsigned short *w = h->wtd_u16.p + (size_t)(c.rows - 1) * N;
    double *const Y = h->filt_Y.p, *const mean = h->filt_sums.p, *const smax = h->filt_sums.p + (size_t)(P * FILT_COLS);
    const dim3 tiles((unsigned)n_tiles, (unsigned)P);
    if (s.ms > 0) {
        hipLaunchKernelGGL(enkf_theta_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, h->psi.p, h->Pdev.p,
                           h->node_tabs.p, (int)h->use_special(), (long long)N, (long long)mpp, (int)D, s, Y, width);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(filter_loglik_kernel, tiles, dim3(FILT_THREADS), 0, h->stream, w, (long long)mpp, (int)D,
                       h->h_wtd_obs[(size_t)row], h->p.dz, h->filt_sigma, s, Y, (long long)n_tiles, h->filt_lmax.p,
                       (const int *)h->filt_win.cap.p, (long long)N, h->fwin_wmax.p);
    HIP_TRY(hipGetLastError());
    if (lagged) w = h->fwin_wmax.p;
    hipLaunchKernelGGL(filter_member_weights_kernel, tiles, dim3(FILT_THREADS), 0, h->stream, w, (long long)mpp, (int)D, s.m,
                       (long long)n_tiles, h->filt_lmax.p, Y, h->filt_qm.p, h->filt_ipart.p, smax);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_tile_partial_kernel, tiles, dim3(FILT_THREADS), 0, h->stream, Y, width, 1, s.m + 1,
                       (const long long *)nullptr, (const double *)nullptr, (long long)mpp, (long long)N, (long long)n_tiles,
                       h->filt_part.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_member_finish_kernel, dim3((unsigned)P), dim3(WAVE), 0, h->stream, h->filt_part.p,
                       h->filt_ipart.p, smax, (long long)n_tiles, (long long)mpp, s, h->filt_sigma,
                       (unsigned long long)h->filt_seed, pbase, key, (unsigned)row, (long long)n_arow, (long long)slot,
                       h->filt_qr.p, h->filt.buf.p, h->filt_surv.p, mean, h->filt_sm.table.buf.p, h->filt_win.table.buf.p);
    HIP_TRY(hipGetLastError());
    return filter_sm_moment(h, s, nullptr, 3, n_tiles, n_arow, slot);
}

// The tempering of a row's weights (hc_set_filter_tempering) after its weight kernels, w being the indices they read.
// The bin path: one kernel, every trial inside the block.  A per-member row (ms > 0 columns between l and e: sensors and
// lagged rows; w then the indices that count a member): trial 0 on the tile sums the weights
// left, then ten pairs of sums and decision enqueued unconditionally -- no host synchronisation; a point that is done
// exits at once -- and the result applied to q_m and the draw.
int filter_temper(hc_handle *h, const unsigned short *w, int ms, int64_t mpp, int64_t n_tiles, int64_t row,
                  const long long *pbase, long long key)
{
    const int64_t D = h->p.dim_d, P = h->n_points, slot = row / h->filt_stride, n_arow = assim_rows(h);
    if (h->filt_trials.ensure((size_t)(P * TEMPER_TRIALS * TEMPER_WIDTH))) return HC_ERR_DEVICE;
    if (ms == 0) {
        hipLaunchKernelGGL(filter_temper_bins_kernel, dim3((unsigned)P), dim3(FILT_THREADS), 0, h->stream, w, (long long)mpp,
                           (int)D, h->h_wtd_obs[(size_t)row], h->p.dz, h->filt_sigma, h->filt_floor,
                           (unsigned long long)h->filt_seed, pbase, key, (unsigned)row, (long long)n_arow, (long long)slot,
                           h->filt_q.p, h->filt_qr.p, h->ftemp.buf.p, h->filt_trials.p);
        HIP_TRY(hipGetLastError());
        return HC_OK;
    }
    if (h->filt_tstate.ensure((size_t)(P * TEMPER_STATE)) || h->filt_tpart.ensure((size_t)(P * n_tiles * 3)))
        return HC_ERR_DEVICE;
    const int width = ms + 2;
    const double *smax = h->filt_sums.p + (size_t)(P * FILT_COLS);
    const dim3 tiles((unsigned)n_tiles, (unsigned)P);
    hipLaunchKernelGGL(filter_temper_decide_kernel, dim3((unsigned)P), dim3(FILT_THREADS), 0, h->stream, h->filt_ipart.p, 4,
                       (long long)n_tiles, 1, h->filt_floor, h->filt_tstate.p, h->filt_trials.p);
    HIP_TRY(hipGetLastError());
    for (int trial = 1; trial < TEMPER_TRIALS; trial++) {
        hipLaunchKernelGGL(filter_temper_sum_kernel, tiles, dim3(FILT_THREADS), 0, h->stream, w, (long long)mpp, (int)D, width,
                           (long long)n_tiles, h->filt_Y.p, smax, h->filt_tstate.p, h->filt_tpart.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(filter_temper_decide_kernel, dim3((unsigned)P), dim3(FILT_THREADS), 0, h->stream, h->filt_tpart.p,
                           3, (long long)n_tiles, 0, h->filt_floor, h->filt_tstate.p, h->filt_trials.p);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(filter_temper_apply_kernel, tiles, dim3(FILT_THREADS), 0, h->stream, w, (long long)mpp, (int)D, width,
                       h->filt_Y.p, smax, h->filt_tstate.p, (unsigned long long)h->filt_seed, pbase, key, (unsigned)row,
                       (long long)n_arow, (long long)slot, h->filt_qm.p, h->filt_qr.p, h->ftemp.buf.p);
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// The rejuvenation of a row's resampled base vectors x [N][D] (hc_set_filter_rejuvenation), in place: two spread passes
// (the EnKF's kernels, unsharded: tile 0 first, each point's first member its own), the moments and the row's entries,
// the move, two spread passes and the entries of what it left.  Everything is enqueued unconditionally -- no host
// synchronisation; a point that is not rejuvenated leaves the move at once and its entries say so.
int filter_rejuvenate(hc_handle *h, double *x, int64_t row, const long long *pbase, long long key)
{
    const int64_t N = h->n_members, D = h->p.dim_d, P = h->n_points, mpp = N / P;
    const int64_t n_tiles = (mpp + ENKF_TILE - 1) / ENKF_TILE, slot = row / h->filt_stride, n_arow = assim_rows(h);
    if (h->rj_part.ensure((size_t)(P * n_tiles * D)) || h->rj_sums.ensure((size_t)(2 * P * D)) ||
        h->rj_mom.ensure((size_t)(3 * P * D)) || h->rj_refused.ensure((size_t)P))
        return HC_ERR_DEVICE;
    double *s1 = h->rj_sums.p, *s2 = s1 + (size_t)(P * D);
    const dim3 tiles((unsigned)n_tiles, (unsigned)P), nodes((unsigned)((D + WAVE - 1) / WAVE * WAVE));
    for (int after = 0; after < 2; after++) {
        for (int sq = 0; sq < 2; sq++) {
            hipLaunchKernelGGL(enkf_spread_kernel, tiles, nodes, 0, h->stream, x, sq ? s1 : nullptr, (long long)mpp, (int)D,
                               (long long)n_tiles, h->rj_part.p, x, (long long)(mpp * D), (long long)mpp, 0LL);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(enkf_finish_kernel, dim3((unsigned)D, (unsigned)P), dim3(ENKF_THREADS), 0, h->stream,
                               h->rj_part.p, (long long)n_tiles, (int)D, sq ? s2 : s1);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(filter_rejuv_diag_kernel, dim3((unsigned)P), nodes, 0, h->stream, x, s1, s2, h->filt_surv.p,
                           h->rj_refused.p, (long long)mpp, (int)D, after, h->rj_mom.p, h->frej.buf.p, (long long)n_arow,
                           (long long)slot);
        HIP_TRY(hipGetLastError());
        if (after) break;
        HIP_TRY(hipMemsetAsync(h->rj_refused.p, 0, (size_t)P * 8, h->stream));
        const unsigned blocks = (unsigned)std::min<size_t>(((size_t)N + 3) / 4, (size_t)h->n_cu * 64);
        hipLaunchKernelGGL(filter_rejuvenate_kernel, dim3(blocks), dim3(256), 0, h->stream, x, h->rj_mom.p, h->filt_surv.p,
                           (long long)N, (long long)mpp, (int)D, h->rj_a, h->rj_h, (unsigned long long)h->filt_seed, pbase, key,
                           (unsigned)row, h->rj_refused.p);
        HIP_TRY(hipGetLastError());
    }
    return HC_OK;
}

// The assimilation at the launch's last row (its water-table indices are wtd_u16's last row): weights, diagnostics and
// draw per point, the member prefix scan, the slot fill, then psi and base gathered into the second buffers and swapped in.
// hc_set_filter_shard: the handle's members are a part of a point of np members; the water-table indices of all of them
// are gathered first (one callback), the same kernels form the whole point's ancestry on every handle, and the gather
// takes the columns of ancestors on other handles from the caller's exchange (filter_shard_resample).
int assimilate(hc_handle *h, const Chunk &c)
{
    const int64_t N = h->n_members, D = h->p.dim_d, P = h->n_points;
    const bool shard = h->fs_n > 0;
    const int64_t first = shard ? h->fs_bounds[(size_t)h->fs_index] : 0;
    const int64_t mpp = shard ? h->fs_bounds[(size_t)h->fs_n] : N / P;
    const int64_t row = c.row0 + c.rows - 1, slot = row / h->filt_stride, n_arow = assim_rows(h);
    const int64_t n_tiles = (mpp + FILT_TILE - 1) / FILT_TILE;
    if (h->filt_q.ensure((size_t)(P * D)) || h->filt_qr.ensure((size_t)(2 * P)) || h->filt_surv.ensure((size_t)P) ||
        h->filt_tiles.ensure((size_t)(P * n_tiles)) || h->filt_anc.ensure((size_t)(P * mpp)) ||
        h->psi_alt.ensure((size_t)(N * D)))
        return HC_ERR_DEVICE;
    if (h->base.ensure((size_t)(N * D)) || h->base_alt.ensure((size_t)(N * D))) return HC_ERR_DEVICE;
    const unsigned short *w = h->wtd_u16.p + (size_t)(c.rows - 1) * N;
    // the draw's key: the point's first global member id (a Philox shard's members are keyed from its own first one)
    long long key = (long long)h->member_offset;
    if (shard) {
        if (h->fs_w.ensure((size_t)mpp) || h->fs_rank.ensure((size_t)mpp) || h->fs_table.ensure((size_t)(6 * h->fs_n)) ||
            h->fs_list.ensure((size_t)(N + h->fs_n - 1)) || h->fs_src.ensure((size_t)N))
            return HC_ERR_DEVICE;
        hipLaunchKernelGGL(filter_shard_index_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, w,
                           (long long)N, h->fs_buf + first);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (int rc = filter_shard_call(h, "gather", h->fs_gather(h->fs_ctx, h->fs_buf, mpp, first, N))) return rc;
        hipLaunchKernelGGL(filter_shard_narrow_kernel, dim3((unsigned)((mpp + 255) / 256)), dim3(256), 0, h->stream,
                           h->fs_buf, (long long)mpp, h->fs_w.p);
        HIP_TRY(hipGetLastError());
        w = h->fs_w.p;
        if (h->philox) key -= first;
    }
    const long long *pbase = P > 1 ? h->point_base.p : nullptr;
    // a row with sensor values (hc_set_filter_soil_moisture; never sharded): a weight per member, and the scan below reads
    // it directly (a null w) in place of the bin's; so does a row with lagged rows of the window (hc_set_filter_window)
    const EnkfRow s = assim_row(h, h->filt_sm, h->filt_win, h->filt_sigma, row);
    const long long *q = h->filt_q.p;
    if (s.m > 0) {
        if (int rc = filter_member_weights(h, c, s, pbase, key)) return rc;
        if (h->filt_floor > 0.0)
            if (int rc = filter_temper(h, s.m > s.ms ? h->fwin_wmax.p : w, s.m, mpp, n_tiles, row, pbase, key)) return rc;
        HIP_TRY(hipMemsetAsync(h->filt_q.p, 0, (size_t)(P * D) * 8, h->stream));
        w = nullptr;
        q = h->filt_qm.p;
    } else {
        hipLaunchKernelGGL(filter_weights_kernel, dim3((unsigned)P), dim3(FILT_THREADS), 0, h->stream, w, (long long)mpp,
                           (int)D, h->h_wtd_obs[(size_t)row], h->p.dz, h->filt_sigma, (unsigned long long)h->filt_seed, pbase,
                           key, (unsigned)row, (long long)n_arow, (long long)slot, h->filt_q.p,
                           h->filt_qr.p, h->filt.buf.p, h->filt_surv.p);
        HIP_TRY(hipGetLastError());
        if (h->filt_floor > 0.0)
            if (int rc = filter_temper(h, w, 0, mpp, n_tiles, row, pbase, key)) return rc;
        if (h->filt_sm.n > 0 || h->filt_win.n > 0) {
            if (h->filt_qm.ensure((size_t)N)) return HC_ERR_DEVICE;
            hipLaunchKernelGGL(filter_expand_weights_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, w,
                               h->filt_q.p, (long long)mpp, (long long)N, (int)D, h->filt_qm.p);
            HIP_TRY(hipGetLastError());
        }
    }
    const dim3 tiles((unsigned)n_tiles, (unsigned)P);
    hipLaunchKernelGGL(filter_tile_sum_kernel, tiles, dim3(FILT_THREADS), 0, h->stream, w, q, (long long)mpp,
                       (int)D, (long long)n_tiles, h->filt_tiles.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_tile_scan_kernel, dim3((unsigned)P), dim3(FILT_THREADS), 0, h->stream, (long long)n_tiles,
                       h->filt_tiles.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(h->filt_anc.p, 0xFF, (size_t)(P * mpp) * 8, h->stream));
    hipLaunchKernelGGL(filter_fill_kernel, tiles, dim3(FILT_THREADS), 0, h->stream, w, q, (long long)mpp, (int)D,
                       (long long)n_tiles, h->filt_tiles.p, h->filt_qr.p, h->filt_anc.p, h->filt_surv.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(filter_survivors_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, h->stream, h->filt_surv.p,
                       (int)P, (long long)n_arow, (long long)slot, h->filt.buf.p);
    HIP_TRY(hipGetLastError());
    if (shard) {
        if (int rc = filter_shard_resample(h, n_tiles)) return rc;
    } else {
        const size_t total = (size_t)N * D;
        const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)h->n_cu * 64);
        hipLaunchKernelGGL(filter_gather_kernel, dim3(blocks), dim3(256), 0, h->stream, h->filt_anc.p, h->psi.p, h->base.p,
                           h->psi_alt.p, h->base_alt.p, (long long)N, (int)D);
        HIP_TRY(hipGetLastError());
        if (h->per_n > 0) {
            // the members' period accumulators travel with their states (the period's path estimate)
            const int K = period_layout(h).K;
            if (h->pacc_alt.ensure((size_t)(N * K))) return HC_ERR_DEVICE;
            const unsigned pblocks = (unsigned)std::min<size_t>(((size_t)N * K + 255) / 256, (size_t)h->n_cu * 64);
            hipLaunchKernelGGL(period_gather_kernel, dim3(pblocks), dim3(256), 0, h->stream, h->filt_anc.p, h->pacc.buf.p,
                               h->pacc_alt.p, (long long)N, K);
            HIP_TRY(hipGetLastError());
            std::swap(h->pacc.buf, h->pacc_alt);
        }
        if (h->upt_layers > 0) {
            // ... and so do their root-uptake accumulators (hc_set_root_uptake)
            const int K = uptake_layout(h).K;
            if (h->uacc_alt.ensure((size_t)(N * K))) return HC_ERR_DEVICE;
            const unsigned ublocks = (unsigned)std::min<size_t>(((size_t)N * K + 255) / 256, (size_t)h->n_cu * 64);
            hipLaunchKernelGGL(period_gather_kernel, dim3(ublocks), dim3(256), 0, h->stream, h->filt_anc.p, h->uacc.buf.p,
                               h->uacc_alt.p, (long long)N, K);
            HIP_TRY(hipGetLastError());
            std::swap(h->uacc.buf, h->uacc_alt);
        }
        if (h->fp_on && h->fp_day >= 0) {
            // ... and so does the perturbed forcing's g, a latent state of the member's trajectory: its two planes as
            // 8-byte words
            if (h->fp_g_alt.ensure((size_t)(2 * N))) return HC_ERR_DEVICE;
            const unsigned gblocks = (unsigned)std::min<size_t>(((size_t)N * 2 + 255) / 256, (size_t)h->n_cu * 64);
            hipLaunchKernelGGL(period_gather_kernel, dim3(gblocks), dim3(256), 0, h->stream, h->filt_anc.p,
                               reinterpret_cast<const long long *>(h->fp_g.p), reinterpret_cast<long long *>(h->fp_g_alt.p),
                               (long long)N, 2);
            HIP_TRY(hipGetLastError());
            std::swap(h->fp_g, h->fp_g_alt);
        }
    }
    if (s.ms > 0) {
        // the sensors' posterior over the resampled slots, theta[anc[k]]: theta is a function of the copied column
        if (int rc = filter_sm_moment(h, s, h->filt_anc.p, 4, n_tiles, n_arow, slot)) return rc;
        if (int rc = filter_sm_moment(h, s, h->filt_anc.p, 5, n_tiles, n_arow, slot)) return rc;
    }
    h->filt_sm.width = s.ms;
    h->filt_ycols = s.m > 0 ? s.m + 2 : 0;
    // the window's buffer is spent: the lagged columns this row took (test hook), every slot empty
    h->filt_win.last.assign(s.sensor + s.ms, s.sensor + s.m);
    std::fill(h->filt_win.row.begin(), h->filt_win.row.end(), (int64_t)-1);
    std::swap(h->psi, h->psi_alt);
    std::swap(h->base, h->base_alt);
    // the rest of this hc_step_rows call launches on the analysis (fill_args took the pointers before the swap)
    h->io_host.psi = h->psi.p;
    if (h->io_host.base_noise) h->io_host.base_noise = h->base.p;
    if (h->rj_delta > 0.0)
        if (int rc = filter_rejuvenate(h, h->base.p, row, pbase, key)) return rc;
    h->filt_done = true;
    return HC_OK;
}

// The smoother (hc_set_filter_smoother): the plane of record slot j into the tables, conditioned on row `cond_row`; the
// plane is then empty
int smoother_emit(hc_handle *h, int64_t j, int64_t cond_row)
{
    const int64_t N = h->n_members, plane = j % (h->smo_lag + 1);
    const long long mpp = N / h->n_points;
    const long long mpb = std::max(HIST_MEMBERS_PER_BLOCK, (mpp + 65535) / 65536);
    const long long slices = (mpp + mpb - 1) / mpb;
    hipLaunchKernelGGL(smoother_emit_kernel, dim3((unsigned)slices, (unsigned)h->n_points), dim3(HIST_THREADS), 0, h->stream,
                       h->smo_w.p + (size_t)plane * N, h->smo_id.p + (size_t)plane * N, mpp, mpb,
                       (long long)smoother_rows(h), (long long)j, (long long)cond_row, (int)h->p.dim_d, h->smo_hist.buf.p,
                       h->smo_paths.buf.p);
    HIP_TRY(hipGetLastError());
    h->smo_row[(size_t)plane] = -1;
    return HC_OK;
}

// ... every live plane of both rings through the ancestor table of the row just resampled, out of place, swapped in
int smoother_gather(hc_handle *h)
{
    SmootherPlanes L{};
    for (size_t k = 0; k < h->smo_row.size(); k++)
        if (h->smo_row[k] >= 0) L.plane[L.n++] = (unsigned char)k;
    if (L.n == 0) return HC_OK;
    const int64_t N = h->n_members;
    hipLaunchKernelGGL(smoother_gather_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, h->filt_anc.p,
                       (long long)N, L, h->smo_w.p, h->smo_id.p, h->smo_w_alt.p, h->smo_id_alt.p);
    HIP_TRY(hipGetLastError());
    std::swap(h->smo_w, h->smo_w_alt);
    std::swap(h->smo_id, h->smo_id_alt);
    return HC_OK;
}

// ... after a launch and its assimilation, if any (`resampled`): the launch's record rows in ascending order, each
// stored from the launch's water-table indices (an unobserved one empties its plane instead), the last one gathered if
// the filter resampled on it, then the plane K record rows back emitted; an assimilation row that is no record row
// gathers only
int smoother_launch(hc_handle *h, const Chunk &c, bool resampled)
{
    const int64_t N = h->n_members, s = h->smo_stride, K = h->smo_lag;
    const int64_t last = c.row0 + c.rows - 1;
    for (int64_t r = std::max<int64_t>(s, (c.row0 + s - 1) / s * s); r <= last; r += s) {
        const int64_t j = r / s, plane = j % (K + 1);
        if (h->h_wtd_obs[(size_t)r] >= 0) {
            hipLaunchKernelGGL(smoother_store_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream,
                               h->wtd_u16.p + (size_t)(r - c.row0) * N, (long long)N, (long long)(N / h->n_points),
                               h->smo_w.p + (size_t)plane * N, h->smo_id.p + (size_t)plane * N);
            HIP_TRY(hipGetLastError());
            h->smo_row[(size_t)plane] = r;
        } else {
            h->smo_row[(size_t)plane] = -1;
        }
        if (r == last && resampled)
            if (int rc = smoother_gather(h)) return rc;
        if (j - K >= 1 && h->smo_row[(size_t)((j - K) % (K + 1))] >= 0)
            if (int rc = smoother_emit(h, j - K, r)) return rc;
    }
    if (resampled && last % s != 0)
        if (int rc = smoother_gather(h)) return rc;
    h->smo_last = last;
    return HC_OK;
}

// The lagged row the launch ended on: every member's y into the window's buffer, by the analysis's own kernel
int enkf_capture(hc_handle *h, const Chunk &c, int slot)
{
    const int64_t N = h->n_members, D = h->p.dim_d;
    if (h->enkf_win.cap.ensure((size_t)(h->enkf_win.n * N))) return HC_ERR_DEVICE;
    const unsigned short *w = h->wtd_u16.p + (size_t)(c.rows - 1) * N;
    hipLaunchKernelGGL(enkf_obs_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, w, h->psi.p, h->Pdev.p,
                       (long long)N, (long long)(N / h->n_points), (int)D, h->p.dz, h->enkf_win.cap.p + (size_t)slot * N, 1);
    HIP_TRY(hipGetLastError());
    h->enkf_win.row[(size_t)slot] = c.row0 + c.rows - 1;
    return HC_OK;
}

// Before a reduction of a sharded analysis (hc_set_enkf_shard): the handle's words of the pass are written, the stream is
// drained and the caller's callback gathers everyone else's into place.  A callback that fails fails the step.
int enkf_exchange(hc_handle *h, double *pass, int64_t n_words, int64_t first_word, int64_t count_words)
{
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int rc = h->shard_fn(h->shard_ctx, pass, n_words, first_word, count_words);
    if (rc) return fail(HC_ERR_DEVICE, "the EnKF shard's exchange callback returned %d (words [%lld, %lld) of %lld)", rc,
                        (long long)first_word, (long long)(first_word + count_words), (long long)n_words);
    return HC_OK;
}

// What the passes of one analysis share: the row, the shape, the tiles and where their partials go.  hc_set_enkf_shard:
// the handle's members are tiles tile0 ... of a point with np members and n_tiles tiles, the partials the passes' global
// layouts in the caller's buffer (part_sq_b behind the prior products it travels with).  Off: np = mpp, tile0 = 0.
struct EnkfPass {
    hc_handle *h;
    const EnkfRow &s;
    int64_t N, D, P, C, n_tiles, my_tiles, tile0, row;
    long long ll_mpp, ll_tiles, ll_np, ll_tile0, n_arow, slot, draw_offset;
    int W, V;
    bool shard, root;
    double dz, z_obs;
    double *part, *part_sq_b, *part_sq;
    dim3 tiles, members, cols_prior;   // a block per tile and point; 256 members a block; a thread per column of (x, Y)
    unsigned blocks;                   // of the member kernels that walk x
    bool taper_x = true;               // the gain tapers C_xY (off: a vector without depth, hc_set_enkf_forcing)

    // the tile partials of one pass (enkf_partial_kernel's arguments), at the handle's tile offset
    hipError_t partials(bool square, const double *x, const double *Y, int width, const double *sums, int Dc, dim3 threads,
                        double *out, double *out_sq) const
    {
        hipLaunchKernelGGL(square ? enkf_partial_kernel<true> : enkf_partial_kernel<false>, tiles, threads, 0, h->stream, x,
                           Y, width, sums, ll_mpp, Dc, ll_tiles, out, out_sq, ll_np, ll_tile0);
        return hipGetLastError();
    }
    // sums[p][c] of a pass of `cols` columns from its tile partials; sharded: the stream drained and the other handles'
    // tiles gathered first (a copy: the partials are the ones one handle would have formed)
    int reduce(double *pass, int64_t cols, double *sums) const
    {
        if (shard)
            if (int rc = enkf_exchange(h, pass, n_tiles * cols, tile0 * cols, my_tiles * cols)) return rc;
        hipLaunchKernelGGL(enkf_finish_kernel, dim3((unsigned)cols, (unsigned)P), dim3(ENKF_THREADS), 0, h->stream, pass,
                           ll_tiles, (int)cols, sums);
        HIP_TRY(hipGetLastError());
        return HC_OK;
    }
    // v.mean_a, then v.sq_a: the sums of x's columns, then of their squared anomalies about that mean, both less each
    // point's first member's column (its own in x, or the copy a sharded analysis's exchange brought)
    int spread(const double *x, EnkfVec &v) const
    {
        for (int sq = 0; sq < 2; sq++) {
            hipLaunchKernelGGL(enkf_spread_kernel, tiles, dim3((unsigned)((D + WAVE - 1) / WAVE * WAVE)), 0, h->stream, x,
                               sq ? v.mean_a.p : nullptr, ll_mpp, (int)D, ll_tiles, part_sq, shard ? h->enkf_first.p : x,
                               shard ? 0LL : ll_mpp * (long long)D, ll_np, ll_tile0);
            HIP_TRY(hipGetLastError());
            if (int rc = reduce(part_sq, D, sq ? v.sq_a.p : v.mean_a.p)) return rc;
        }
        return HC_OK;
    }
};

// One vector's part of the analysis, in place on x [N][D]: the sums of (x, Y), then the products of their anomalies with
// Y's (two passes over x); the gain; the update (one read + write of x; hc_set_enkf_method: the square-root scheme's
// own, from the reduced gain and the mean's increment the gain kernel adds); with alpha > 0 the relaxation to prior
// spread -- the analysis columns' sums, their squared anomalies (two more passes), the factors, the relaxed columns (one
// read + write).  The caller chooses: `square`, whether the second prior pass takes the squared anomalies along (the
// relaxation needs them; a table of the prior std does regardless); st, sst, wst, the EnKF's, the sensors' and the
// window's table for the gain kernel's prior diagnostics (NULL: none); `refused`, per member whether the update or the
// relaxation refused its vector (NULL: not kept; both read Ypost's rejected flag either way).  STATE (x is psi) chooses
// the member kernels' instance, the draws -- made between the gain and the stochastic update of the state alone, any
// other vector reuses them -- and whether the update writes y into Ypost: the state's does unless a relaxation follows
// and writes it.  A sharded analysis exchanges before every reduction and, under relaxation, brings the point's first
// member's column to every handle (enkf_first_member_kernel, one more exchange, enkf_first); the spread and the factors
// then read that copy with stride 0 instead of x with stride mpp D.  The noise field's table and the posterior are
// enkf_analyse's.  (The gain, the square-root update and the relaxation's factors take N_p = np; the latter two also
// index the points by m / N_p: a sharded handle holds one point, m / np = 0.)
template <bool STATE>
int enkf_vector(const EnkfPass &g, double *x, EnkfVec &v, double alpha, bool square, double *st, double *sst, double *wst,
                double *refused)
{
    hc_handle *h = g.h;
    const EnkfRow &s = g.s;
    const int64_t N = g.N, D = g.D, P = g.P, C = g.C;
    const int W = g.W, V = g.V;
    const bool relax = alpha > 0.0;
    const int want_y = STATE && !relax ? 1 : 0;
    int rc = HC_OK;
    HIP_TRY(g.partials(false, x, h->enkf_Y.p, W, nullptr, (int)D, g.cols_prior, g.part, nullptr));
    if ((rc = g.reduce(g.part, C, v.s1.p))) return rc;
    HIP_TRY(g.partials(square, x, h->enkf_Y.p, W, v.s1.p, (int)D, g.cols_prior, g.part, square ? g.part_sq_b : nullptr));
    if ((rc = g.reduce(g.part, C * W, v.s2.p))) return rc;
    if (square && (rc = g.reduce(g.part_sq_b, D, v.sq_b.p))) return rc;
    hipLaunchKernelGGL(enkf_gain_kernel, dim3((unsigned)P), dim3((unsigned)((D + WAVE - 1) / WAVE * WAVE)), 0, h->stream,
                       v.s1.p, v.s2.p, g.ll_np, (int)D, s, h->enkf_sigma, h->enkf_loc, g.z_obs, g.dz, v.gain.p, st, sst,
                       g.n_arow, g.slot, g.root ? v.rgain.p : nullptr, g.root ? v.dbar.p : nullptr, wst, g.taper_x ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (g.root) {
        hipLaunchKernelGGL(enkf_sqrt_update_kernel<STATE>, dim3(g.blocks), dim3(256), 0, h->stream, x, h->enkf_Y.p,
                           v.rgain.p, v.dbar.p, v.s1.p, h->Pdev.p, (long long)N, g.ll_np, (int)D, g.dz, W, V, want_y,
                           h->enkf_Ypost.p, refused);
    } else {
        if (STATE) {
            hipLaunchKernelGGL(enkf_draw_kernel, g.members, dim3(256), 0, h->stream, (long long)N, g.ll_mpp,
                               (unsigned long long)h->enkf_seed, P > 1 ? h->point_base.p : nullptr, g.draw_offset,
                               (unsigned)g.row, s.n, h->enkf_eps.p, h->enkf_eps_s.p);
            HIP_TRY(hipGetLastError());
            if (s.m > s.ms) {
                hipLaunchKernelGGL(enkf_window_draw_kernel, g.members, dim3(256), 0, h->stream, (long long)N, g.ll_mpp,
                                   (unsigned long long)h->enkf_seed, P > 1 ? h->point_base.p : nullptr, g.draw_offset, s,
                                   h->enkf_eps_w.p);
                HIP_TRY(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(enkf_update_kernel<STATE>, dim3(g.blocks), dim3(256), 0, h->stream, x, h->enkf_Y.p, v.gain.p,
                           h->Pdev.p, (long long)N, g.ll_mpp, (int)D, g.dz, g.z_obs, h->enkf_sigma, s, h->enkf_eps.p,
                           h->enkf_eps_s.p, h->enkf_eps_w.p, want_y, h->enkf_Ypost.p, refused);
    }
    HIP_TRY(hipGetLastError());
    if (!relax) return HC_OK;
    if (g.shard) {
        // the point's first member's analysis column, from the handle that holds it, to every handle
        const bool mine = h->shard_first == 0;
        if (mine) {
            hipLaunchKernelGGL(enkf_first_member_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, h->stream, x,
                               (int)D, h->shard_buf);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = enkf_exchange(h, h->shard_buf, D, 0, mine ? D : 0))) return rc;
        HIP_TRY(hipMemcpyAsync(h->enkf_first.p, h->shard_buf, (size_t)D * 8, hipMemcpyDeviceToDevice, h->stream));
    }
    if ((rc = g.spread(x, v))) return rc;
    hipLaunchKernelGGL(enkf_relax_factor_kernel, dim3((unsigned)((P * D + 255) / 256)), dim3(256), 0, h->stream, v.sq_b.p,
                       v.sq_a.p, v.mean_a.p, g.shard ? h->enkf_first.p : x, v.gain.p, (long long)P, g.ll_np, (int)D, W, alpha,
                       v.relax.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(enkf_relax_kernel<STATE>, dim3(g.blocks), dim3(256), 0, h->stream, x, v.relax.p + (size_t)(3 * P * D),
                       v.relax.p + (size_t)(2 * P * D), h->Pdev.p, (long long)N, g.ll_mpp, (int)D, g.dz, V, h->enkf_Ypost.p,
                       refused);
    HIP_TRY(hipGetLastError());
    return HC_OK;
}

// The EnKF's analysis at the launch's last row (its water-table indices are wtd_u16's last row), m' = 1 + s.m
// observations per member: y and theta per member; psi's part (enkf_vector: the prior diagnostics and the posterior y are
// its); with hc_set_enkf_noise_field the base vectors z's part, from the same Y, factor, innovations and draws (Y is
// still the forecast's; Ypost holds the rejected flags) with its own alpha, then the noise field's table; the posterior
// theta, the sums over (y, theta, rejected) and diagnostics.  Scratch is sized by the record's largest m', Wx.  With
// hc_set_enkf_shard every partial pass writes the handle's tiles into the pass's global layout in the caller's buffer
// and every reduction gathers the other handles' first (one callback each), so the sums -- and everything after them
// -- are those of the one handle that holds every member.
int enkf_analyse(hc_handle *h, const Chunk &c, const EnkfRow &s)
{
    const int64_t N = h->n_members, D = h->p.dim_d, P = h->n_points, mpp = N / P;
    const int64_t row = c.row0 + c.rows - 1, slot = row / h->enkf_stride, n_arow = assim_rows(h);
    const bool shard = h->shard_global > 0;
    const int64_t np = shard ? h->shard_global : mpp, tile0 = shard ? h->shard_first / ENKF_TILE : 0;
    const int64_t my_tiles = (mpp + ENKF_TILE - 1) / ENKF_TILE, n_tiles = (np + ENKF_TILE - 1) / ENKF_TILE;
    const int W = s.m + 1, V = s.ms + 2, mw = s.m - s.ms;
    const int64_t C = D + W, Wx = 1 + h->enkf_sm.n + h->enkf_win.n, Cx = D + Wx;
    if (shard && h->shard_words < shard_words_needed(h, np))
        return fail(HC_ERR_ARG, "the shard's buffer holds %lld doubles, the analysis needs %lld (sensors or a window set "
                    "after hc_set_enkf_shard: set the shard again)", (long long)h->shard_words,
                    (long long)shard_words_needed(h, np));
    const int64_t cols_x = std::max(Cx * Wx, (Wx + 1) * (Wx + 1));   // the widest pass: the prior products or the posterior's
    const bool root = h->enkf_method == 1, relax = h->enkf_alpha > 0.0;
    if (h->enkf_Y.ensure((size_t)(N * Wx)) || h->enkf_eps.ensure((size_t)N) ||
        h->enkf_eps_s.ensure((size_t)(N * h->enkf_sm.n)) || h->enkf_eps_w.ensure((size_t)(N * h->enkf_win.n)) ||
        h->enkf_Ypost.ensure((size_t)(N * (Wx + 1))) || h->enkf_psi.ensure(P, D, Wx, cols_x, root, relax, relax) ||
        (!shard && h->enkf_part.ensure((size_t)(P * n_tiles * cols_x))) ||
        (relax && (shard ? h->enkf_first.ensure((size_t)D) : h->enkf_part_sq.ensure((size_t)(P * n_tiles * D)))))
        return HC_ERR_DEVICE;
    if (h->enkf_nz) {
        if (shard) return fail(HC_ERR_ARG, "the noise field with a sharded analysis: the exchanged partials cover psi only");
        if (h->enkf_part_sq.ensure((size_t)(P * n_tiles * D)) || h->nz_rej.ensure((size_t)N) || h->nz_rejsum.ensure((size_t)P) ||
            h->enkf_z.ensure(P, D, Wx, Cx * Wx, root, true, h->enkf_nz_alpha > 0.0))
            return HC_ERR_DEVICE;
    }
    if (h->enkf_fg) {
        if (shard) return fail(HC_ERR_ARG, "the forcing analysis with a sharded analysis: the exchanged partials cover psi only");
        if (h->enkf_part_sq.ensure((size_t)(P * n_tiles * D)) || h->fg_x.ensure((size_t)(2 * N)) ||
            h->fg_rej.ensure((size_t)N) || h->fg_rejsum.ensure((size_t)P) ||
            h->enkf_gv.ensure(P, 2, Wx, (2 + Wx) * Wx, root, true, h->enkf_fg_alpha > 0.0))
            return HC_ERR_DEVICE;
    }
    const unsigned short *w = h->wtd_u16.p + (size_t)(c.rows - 1) * N;
    const double dz = h->p.dz;
    const int special = (int)h->use_special();
    const long long ll_mpp = (long long)mpp, ll_np = (long long)np;
    const dim3 members((unsigned)((N + 255) / 256)), cols_post((unsigned)WAVE);
    const EnkfPass g{h, s, N, D, P, C, n_tiles, my_tiles, tile0, row,
                     ll_mpp, (long long)n_tiles, ll_np, (long long)tile0, (long long)n_arow, (long long)slot,
                     (long long)(shard ? h->shard_first : h->member_offset),
                     W, V, shard, root, dz, (double)h->h_wtd_obs[(size_t)row] * dz,
                     shard ? h->shard_buf : h->enkf_part.p,
                     shard ? h->shard_buf + (size_t)(n_tiles * C * W) : h->enkf_part_sq.p,
                     shard ? h->shard_buf : h->enkf_part_sq.p,
                     dim3((unsigned)my_tiles, (unsigned)P), members, dim3((unsigned)((C + WAVE - 1) / WAVE * WAVE)),
                     (unsigned)std::min<int64_t>((N + 3) / 4, (int64_t)h->n_cu * 8)};
    int rc = HC_OK;
    hipLaunchKernelGGL(enkf_obs_kernel, members, dim3(256), 0, h->stream, w, h->psi.p, h->Pdev.p, (long long)N, ll_mpp,
                       (int)D, dz, h->enkf_Y.p, W);
    HIP_TRY(hipGetLastError());
    if (s.ms > 0) {
        hipLaunchKernelGGL(enkf_theta_kernel, members, dim3(256), 0, h->stream, h->psi.p, h->Pdev.p, h->node_tabs.p, special,
                           (long long)N, ll_mpp, (int)D, s, h->enkf_Y.p, W);
        HIP_TRY(hipGetLastError());
    }
    if (mw > 0) {
        hipLaunchKernelGGL(enkf_window_gather_kernel, members, dim3(256), 0, h->stream, h->enkf_win.cap.p, (long long)N, s,
                           h->enkf_Y.p, W);
        HIP_TRY(hipGetLastError());
    }
    double *st = h->enkf.buf.p, *sst = h->enkf_sm.table.buf.p, *wst = h->enkf_win.table.buf.p;
    if ((rc = enkf_vector<true>(g, h->psi.p, h->enkf_psi, h->enkf_alpha, relax, st, sst, wst, nullptr))) return rc;
    if (h->enkf_nz) {
        // the noise field, then for its table the spread of what the update and the relaxation, if any, left (never
        // sharded: part_sq is the handle's own) and the refused vectors' count
        double *const z = h->base.p;
        EnkfVec &v = h->enkf_z;
        if ((rc = enkf_vector<false>(g, z, v, h->enkf_nz_alpha, true, nullptr, nullptr, nullptr, h->nz_rej.p))) return rc;
        if ((rc = g.spread(z, v))) return rc;
        HIP_TRY(g.partials(false, nullptr, h->nz_rej.p, 1, nullptr, 0, cols_post, g.part, nullptr));
        if ((rc = g.reduce(g.part, 1, h->nz_rejsum.p))) return rc;
        hipLaunchKernelGGL(enkf_noise_diag_kernel, dim3((unsigned)((P * D + 255) / 256)), dim3(256), 0, h->stream, v.s1.p,
                           v.sq_b.p, v.mean_a.p, v.sq_a.p, z, h->nz_rejsum.p, (long long)P, ll_np, (int)D, W,
                           h->enkf_nzt.buf.p, (long long)n_arow, (long long)slot);
        HIP_TRY(hipGetLastError());
        h->nz_done = true;
    }
    if (h->enkf_fg) {
        // the members' forcing state g of the row's day, as the columns x [N][2] of a pass with D = 2 and no taper on C_gY;
        // then, as for the noise field, the spread of what was left and the refused count for the table; the analysed
        // streams go back into the carried buffer, which the next launch starts from
        if (!h->fp_on || h->fp_day != row / HC_FORCING_DAY_ROWS || !h->fp_g.p)
            return fail(HC_ERR_ARG, "the forcing analysis of row %lld: the members' forcing state stands at day %lld",
                        (long long)row, (long long)h->fp_day);
        EnkfPass gf = g;
        gf.D = 2;
        gf.C = 2 + W;
        gf.cols_prior = dim3((unsigned)((gf.C + WAVE - 1) / WAVE * WAVE));
        gf.taper_x = false;
        EnkfVec &v = h->enkf_gv;
        double *const x = h->fg_x.p;
        const int act0 = h->fp_sigma[0] > 0.0 ? 1 : 0, act1 = h->fp_sigma[1] > 0.0 ? 1 : 0;
        hipLaunchKernelGGL(enkf_forcing_gather_kernel, members, dim3(256), 0, h->stream, h->fp_g.p, (long long)N, x);
        HIP_TRY(hipGetLastError());
        if ((rc = enkf_vector<false>(gf, x, v, h->enkf_fg_alpha, true, nullptr, nullptr, nullptr, h->fg_rej.p))) return rc;
        if ((rc = gf.spread(x, v))) return rc;
        HIP_TRY(gf.partials(false, nullptr, h->fg_rej.p, 1, nullptr, 0, cols_post, gf.part, nullptr));
        if ((rc = gf.reduce(gf.part, 1, h->fg_rejsum.p))) return rc;
        hipLaunchKernelGGL(enkf_forcing_diag_kernel, dim3((unsigned)((2 * P + 63) / 64)), dim3(64), 0, h->stream, v.s1.p,
                           v.sq_b.p, v.mean_a.p, v.sq_a.p, x, h->fg_rejsum.p, (long long)P, ll_np, W, act0, act1,
                           h->enkf_fgt.buf.p, (long long)n_arow, (long long)slot);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(enkf_forcing_scatter_kernel, members, dim3(256), 0, h->stream, x, (long long)N, act0, act1,
                           h->fp_g.p);
        HIP_TRY(hipGetLastError());
        h->fg_done = true;
    }
    if (s.ms > 0) {
        hipLaunchKernelGGL(enkf_theta_kernel, members, dim3(256), 0, h->stream, h->psi.p, h->Pdev.p, h->node_tabs.p, special,
                           (long long)N, ll_mpp, (int)D, s, h->enkf_Ypost.p, V);
        HIP_TRY(hipGetLastError());
    }
    // posterior: the same two passes over (y, theta, rejected) alone
    double *const s1 = h->enkf_psi.s1.p, *const s2 = h->enkf_psi.s2.p;
    HIP_TRY(g.partials(false, nullptr, h->enkf_Ypost.p, V, nullptr, 0, cols_post, g.part, nullptr));
    if ((rc = g.reduce(g.part, V, s1))) return rc;
    HIP_TRY(g.partials(false, nullptr, h->enkf_Ypost.p, V, s1, 0, cols_post, g.part, nullptr));
    if ((rc = g.reduce(g.part, V * V, s2))) return rc;
    hipLaunchKernelGGL(enkf_post_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, h->stream, s1, s2, (long long)P,
                       ll_np, s, st, sst, (long long)n_arow, (long long)slot);
    HIP_TRY(hipGetLastError());
    h->enkf_done = true;
    h->enkf_width = W;
    h->enkf_last_method = h->enkf_method;
    h->enkf_last_relaxed = relax;
    h->enkf_sm.width = s.ms > 0 ? 1 + s.ms : 0;
    h->enkf_win.last.assign(s.sensor + s.ms, s.sensor + s.m);
    std::fill(h->enkf_win.row.begin(), h->enkf_win.row.end(), (int64_t)-1);   // the captured rows are spent
    return HC_OK;
}

// After the launches of a call: a split-column mailbox exchange that timed out invalidates the results.  An attempt that
// exhausts the kernel's iteration budget is abandoned like a solve that gave up (the x0.8 retry rule applies); it is
// counted ([2], last place in [3]) and only fatal on request.
int check_counters(hc_handle *h)
{
    unsigned long long cnt[6];
    HIP_TRY(hipMemcpy(cnt, h->counters.p, sizeof(cnt), hipMemcpyDeviceToHost));
    if (cnt[5] != 0)
        return fail(HC_ERR_DEVICE, "split-column kernel: %llu mailbox exchanges timed out (internal error; results are invalid)", cnt[5]);
    if (cnt[2] != 0 && h->strict_guard)
        return fail(HC_ERR_DEVICE, "%llu BDF attempts hit the kernel's iteration guard (last: member %llu, row %llu)",
                    cnt[2], cnt[3] >> 24, cnt[3] & 0xFFFFFFull);
    return HC_OK;
}
}  // namespace

extern "C" {

int hc_step_rows(hc_handle *h, hc_step_args *a)
{
    if (!h || !a) return fail(HC_ERR_ARG, "hc_step_rows: NULL argument");
    StepArgs A;
    int rc = fill_args(h, A);
    if (rc) return rc;
    if (a->n_rows < 0) return fail(HC_ERR_ARG, "n_rows < 0");
    if (a->spinup && a->accumulate_moments)
        return fail(HC_ERR_ARG, "spin-up solves have no forcing row of their own: accumulate_moments must be 0");
    if (a->spinup) {
        if (a->row_begin < 0 || a->row_begin >= h->n_rows) return fail(HC_ERR_ARG, "spin-up forcing row out of range");
    } else if (a->row_begin < 1 || a->row_begin + a->n_rows > h->n_rows) {
        return fail(HC_ERR_ARG, "rows [%lld, %lld) outside [1, %lld)", (long long)a->row_begin,
                    (long long)(a->row_begin + a->n_rows), (long long)h->n_rows);
    }
    HIP_TRY(hipSetDevice(h->device));
    a->kernel_ms = 0.0;
    a->launches = 0;
    // profile statistics (hc_set_profile_stats) and water-table histograms (hc_set_wtd_hist, read from wtd_u16 after
    // each launch): spin-up solves accumulate nothing
    const bool prof_on = h->prof_stride > 0 && !a->spinup, hist_on = h->hist_stride > 0 && !a->spinup;
    if ((prof_on && (rc = ensure_prof(h))) || (hist_on && (rc = ensure_hist(h)))) return rc;
    if (prof_on && h->thist_bins > 0 && (rc = ensure_thist(h))) return rc;
    if (prof_on && h->stor_layers > 0 && (rc = ensure_stor(h))) return rc;
    if (prof_on && h->cov_stride > 0 && (rc = ensure_cov(h))) return rc;
    const bool cond_on = prof_on && h->cond_on;           // conductivity statistics (hc_set_conductivity_stats)
    if (cond_on && (rc = ensure_cond(h))) return rc;
    const bool per_on = h->per_n > 0 && !a->spinup;       // period totals (hc_set_period_totals)
    if (per_on && (rc = ensure_period(h))) return rc;
    if (per_on && h->upt_layers > 0 && ((rc = ensure_uptake(h)) || (rc = ensure_mid_tabs(h)))) return rc;
    // the particle filter (hc_set_filter): spin-up solves are never filtered
    if (a->spinup && h->filt_host())
        return fail(HC_ERR_ARG, "spin-up solves with the particle filter on in a Philox run: set the filter after the spin-up");
    if (a->spinup && h->corr_host())
        return fail(HC_ERR_ARG, "spin-up solves with a noise correlation set: set the correlation after the spin-up");
    if (a->spinup && h->noise_host())
        return fail(HC_ERR_ARG, "spin-up solves with the EnKF's noise field on in a Philox run: set it after the spin-up");
    const bool filt_on = h->filt_stride > 0 && !a->spinup;
    const bool enkf_on = h->enkf_stride > 0 && !a->spinup;   // (the EnKF: spin-up solves are never analysed either)
    if ((filt_on && (rc = ensure_filter(h))) || (enkf_on && (rc = ensure_enkf(h)))) return rc;
    if (enkf_on && h->enkf_nz && (rc = ensure_nz(h))) return rc;
    if (enkf_on && h->enkf_fg && (rc = ensure_fg(h))) return rc;
    const Assim da = assim(h);                               // whichever is on: its record's and its window's tables
    const bool da_on = filt_on || enkf_on;
    if (da_on && da.sm.n > 0 && (rc = da.ensure_sm(h))) return rc;
    if (filt_on && h->filt_floor > 0.0 && (rc = ensure_ftemp(h))) return rc;
    if (filt_on && h->rj_delta > 0.0 && (rc = ensure_frej(h))) return rc;
    if (da_on && da.win.n > 0 && (rc = da.ensure_win(h))) return rc;
    const bool smo_on = filt_on && h->smo_stride > 0;        // the smoother (hc_set_filter_smoother)
    if (smo_on && (rc = ensure_smoother(h))) return rc;
    int64_t fresh_consumed = 0;
    for (int64_t done = 0; done < a->n_rows;) {
        const Chunk c = plan_chunk(h, a, done, prof_on);
        int n_fresh = 0;
        if ((rc = stage_noise(h, a, c, fresh_consumed, n_fresh))) return rc;
        h->cond_fresh_last = n_fresh - 1;
        if ((rc = launch_chunk(h, A, a, c, prof_on || per_on, cond_on))) return rc;
        if ((rc = accumulate(h, A, a, c, prof_on, hist_on))) return rc;
        if ((rc = copy_outputs(h, a, c, done))) return rc;
        const int64_t last = c.row0 + c.rows - 1;
        if (filt_on && is_assimilation_row(h, last) && (rc = assimilate(h, c))) return rc;
        if (smo_on && (rc = smoother_launch(h, c, is_assimilation_row(h, last)))) return rc;
        if (enkf_on && is_assimilation_row(h, last) &&
            (rc = enkf_analyse(h, c, assim_row(h, h->enkf_sm, h->enkf_win, h->enkf_sigma, last))))
            return rc;
        if (const int wslot = da_on ? window_slot(h, last) : -1; wslot >= 0)
            if ((rc = filt_on ? filter_capture(h, c, wslot) : enkf_capture(h, c, wslot))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        a->kernel_ms += ms;
        a->launches++;
        fresh_consumed += n_fresh;
        done += c.rows;
        if (h->n_points > 1 && !a->spinup) {
            // what each point cost in this launch orders the next one: costliest point first (results do not depend on it)
            std::vector<unsigned long long> cost((size_t)h->n_points);
            HIP_TRY(hipMemcpy(cost.data(), h->point_cost.p, cost.size() * 8, hipMemcpyDeviceToHost));
            for (int k = 0; k < h->n_points; k++) h->cost_total[(size_t)k] += cost[(size_t)k];
            if (!h->fixed_order)
                std::stable_sort(h->order_host.begin(), h->order_host.end(),
                                 [&](int x, int y) { return cost[(size_t)x] > cost[(size_t)y]; });
        }
    }
    return check_counters(h);
}

int hc_spinup(hc_handle *h, hc_spinup_args *a)
{
    if (!h || !a || !a->iterations_out) return fail(HC_ERR_ARG, "hc_spinup: NULL argument");
    StepArgs A;
    int rc = fill_args(h, A);
    if (rc) return rc;
    if (a->forcing_row < 0 || a->forcing_row >= h->n_rows) return fail(HC_ERR_ARG, "spin-up forcing row out of range");
    if (a->max_iterations < 1 || a->max_iterations > 1000000) return fail(HC_ERR_ARG, "max_iterations out of range");
    if (h->filt_host())
        return fail(HC_ERR_ARG, "hc_spinup with the particle filter on in a Philox run: set the filter after the spin-up");
    if (h->corr_host())
        return fail(HC_ERR_ARG, "hc_spinup with a noise correlation set: set the correlation after the spin-up");
    if (h->noise_host())
        return fail(HC_ERR_ARG, "hc_spinup with the EnKF's noise field on in a Philox run: set it after the spin-up");
    HIP_TRY(hipSetDevice(h->device));
    const int64_t N = h->n_members;
    if (h->spin_iters.ensure((size_t)N)) return HC_ERR_DEVICE;
    h->io_host.row_begin = a->forcing_row;
    h->io_host.spin_iters = h->spin_iters.p;
    A.n_rows = a->max_iterations;
    A.spinup = 1;
    A.spin_stop = 1;
    A.spin_zwtd = a->zwtd_cm;
    A.spin_z0 = a->z0_cm;
    A.spin_dz = h->p.dz;
    rc = push_io(h);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    rc = launch_step(h, A);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipMemcpyAsync(a->iterations_out, h->spin_iters.p, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    a->kernel_ms = ms;
    return check_counters(h);
}

int hc_get_counters(hc_handle *h, uint64_t *out4)
{
    if (!h || !out4) return fail(HC_ERR_ARG, "hc_get_counters: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out4, h->counters.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HC_OK;
}

#ifdef HC_PROFILE
extern "C" int hc_debug_trace(hc_handle *h, double *out, int64_t n)
{
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!h->trace.p) return fail(HC_ERR_ARG, "no trace (set HYDROCOL_DEBUG_TRACE)");
    HIP_TRY(hipMemcpy(out, h->trace.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}
extern "C" int hc_debug_profile(hc_handle *h, uint64_t *out32)
{
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out32, h->counters.p + 8, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HC_OK;
}
extern "C" int hc_debug_profile_counts(hc_handle *h, uint64_t *out32)      // entries into each region
{
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out32, h->counters.p + 64, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HC_OK;
}
extern "C" int hc_debug_profile_subcounts(hc_handle *h, uint64_t *out32)   // entries into sub-regions 32..63
{
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out32, h->counters.p + 96, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HC_OK;
}
#endif

int hc_synchronize(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return HC_OK;
}

int hc_get_moments(hc_handle *h, int64_t *moments)
{
    if (!h || !moments) return fail(HC_ERR_ARG, "hc_get_moments: bad argument");
    return table_copy(h, h->moments, ensure_moments, hipMemcpyDeviceToHost, moments);
}

int hc_export_moments(hc_handle *h, void *device_dst)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_moments: bad argument");
    return table_copy(h, h->moments, ensure_moments, hipMemcpyDeviceToDevice, device_dst);
}

int hc_set_moments(hc_handle *h, const int64_t *moments)
{
    if (!h || !moments) return fail(HC_ERR_ARG, "hc_set_moments: bad argument");
    return table_copy(h, h->moments, ensure_moments, hipMemcpyHostToDevice, const_cast<int64_t *>(moments));
}

int hc_reset_moments(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_moments: bad argument");
    return table_reset(h, h->moments, ensure_moments);
}

int hc_set_profile_stats(hc_handle *h, int32_t stride)
{
    if (!h || stride < 0) return fail(HC_ERR_ARG, "hc_set_profile_stats: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->prof_stride = stride;
    h->prof.release();           // re-created, zeroed, when on
    h->thist_bins = 0;           // the soil-moisture histograms are keyed to the profile rows: off
    h->thist.release();
    h->stor_layers = h->stor_bins = 0;       // and so is the layer storage
    h->stor.release(), h->shist.release();
    h->cov_stride = 0;           // ... and the theta covariance
    h->cov.release(), h->cov_q.release();
    cond_off(h);                 // ... and the conductivity statistics
    return stride == 0 ? HC_OK : ensure_prof(h);
}

int hc_get_profile_stats_words(hc_handle *h, int64_t *n_words)
{
    if (!h || !n_words) return fail(HC_ERR_ARG, "hc_get_profile_stats_words: bad argument");
    if (int rc = ensure_prof(h)) return rc;
    *n_words = h->prof.n;
    return HC_OK;
}

int hc_profile_snapshot(hc_handle *h, int64_t row)
{
    if (!h) return fail(HC_ERR_ARG, "hc_profile_snapshot: NULL handle");
    StepArgs A;
    int rc = fill_args(h, A);
    if (rc) return rc;
    if (int rc2 = ensure_prof(h)) return rc2;
    if (row < 0 || row >= h->n_rows || row % h->prof_stride != 0)
        return fail(HC_ERR_ARG, "hc_profile_snapshot: row %lld is not a profile row (stride %d, %lld rows)", (long long)row,
                    h->prof_stride, (long long)h->n_rows);
    HIP_TRY(hipSetDevice(h->device));
    if (h->thist_bins > 0)
        if (int rc2 = ensure_thist(h)) return rc2;
    if (h->stor_layers > 0)
        if (int rc2 = ensure_stor(h)) return rc2;
    if (h->cov_stride > 0)
        if (int rc2 = ensure_cov(h)) return rc2;
    if (h->cond_on)
        if (int rc2 = ensure_cond(h)) return rc2;
    if (int rc2 = launch_profile(h, A, prof_layout(h), h->psi.p, row, 1)) return rc2;
    if (h->thist_bins > 0)
        if (int rc2 = launch_theta_hist(h, A, prof_layout(h), h->psi.p, row, 1)) return rc2;
    if (h->stor_layers > 0)
        if (int rc2 = launch_layer_storage(h, A, prof_layout(h), h->psi.p, row, 1)) return rc2;
    if (h->cov_stride > 0)
        if (int rc2 = launch_theta_cov(h, A, prof_layout(h), h->psi.p, row, 1)) return rc2;
    if (h->cond_on)
        if (int rc2 = launch_conductivity(h, A, prof_layout(h), h->psi.p, row, 1, nullptr, nullptr)) return rc2;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return HC_OK;
}

int hc_get_profile_stats(hc_handle *h, int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_profile_stats: bad argument");
    return table_copy(h, h->prof, ensure_prof, hipMemcpyDeviceToHost, table, n_words, "hc_get_profile_stats");
}

int hc_set_profile_stats_tables(hc_handle *h, const int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_profile_stats_tables: bad argument");
    return table_copy(h, h->prof, ensure_prof, hipMemcpyHostToDevice, const_cast<int64_t *>(table), n_words,
                      "hc_set_profile_stats_tables");
}

int hc_export_profile_stats(hc_handle *h, void *device_dst, int64_t n_words)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_profile_stats: bad argument");
    return table_copy(h, h->prof, ensure_prof, hipMemcpyDeviceToDevice, device_dst, n_words, "hc_export_profile_stats");
}

int hc_reset_profile_stats(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_profile_stats: bad argument");
    return table_reset(h, h->prof, ensure_prof);
}

int hc_get_profile_overflow(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_profile_overflow: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_prof(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->prof.buf.p + prof_layout(h).ovf, 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_wtd_hist(hc_handle *h, int32_t stride)
{
    if (!h || stride < 0) return fail(HC_ERR_ARG, "hc_set_wtd_hist: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->hist_stride = stride;
    h->hist.release();           // re-created, zeroed, when on
    const int rc = stride == 0 ? HC_OK : ensure_hist(h);
    if (rc != HC_OK) h->hist_stride = 0, h->hist.release();      // refused: off
    return rc;
}

int hc_get_wtd_hist(hc_handle *h, int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_wtd_hist: bad argument");
    return table_copy(h, h->hist, ensure_hist, hipMemcpyDeviceToHost, table, n_entries, "hc_get_wtd_hist");
}

int hc_set_wtd_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_wtd_hist_table: bad argument");
    return table_copy(h, h->hist, ensure_hist, hipMemcpyHostToDevice, const_cast<int32_t *>(table), n_entries,
                      "hc_set_wtd_hist_table");
}

int hc_reset_wtd_hist(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_wtd_hist: bad argument");
    return table_reset(h, h->hist, ensure_hist);
}

int hc_set_theta_hist(hc_handle *h, int32_t n_bins)
{
    if (!h) return fail(HC_ERR_ARG, "hc_set_theta_hist: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->thist.release();          // re-created, zeroed, when on
    h->thist_bins = 0;
    if (n_bins == 0) return HC_OK;
    if (n_bins != 32 && n_bins != 64 && n_bins != 128)
        return fail(HC_ERR_ARG, "hc_set_theta_hist: %d bins (32, 64 or 128; 0 = off)", (int)n_bins);
    h->thist_bins = n_bins;
    const int rc = ensure_thist(h);          // (its refusals come before anything is allocated)
    if (rc != HC_OK) h->thist_bins = 0, h->thist.release();      // refused: off
    return rc;
}

int hc_get_theta_hist(hc_handle *h, int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_theta_hist: bad argument");
    return table_copy(h, h->thist, ensure_thist, hipMemcpyDeviceToHost, table, n_entries, "hc_get_theta_hist");
}

int hc_set_theta_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_theta_hist_table: bad argument");
    return table_copy(h, h->thist, ensure_thist, hipMemcpyHostToDevice, const_cast<int32_t *>(table), n_entries,
                      "hc_set_theta_hist_table");
}

int hc_reset_theta_hist(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_theta_hist: bad argument");
    return table_reset(h, h->thist, ensure_thist);
}

int hc_get_theta_hist_outside(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_theta_hist_outside: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_thist(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->thist.buf.p + (h->thist.n - 2), 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_theta_hist_bins(hc_handle *h, int32_t *n_bins)
{
    if (!h || !n_bins) return fail(HC_ERR_ARG, "hc_get_theta_hist_bins: bad argument");
    *n_bins = h->thist_bins;
    return HC_OK;
}

int hc_set_layer_storage(hc_handle *h, int32_t n_layers, const int32_t *ranges, int32_t n_bins)
{
    if (!h || (n_layers > 0 && !ranges)) return fail(HC_ERR_ARG, "hc_set_layer_storage: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->stor.release(), h->shist.release();   // re-created, zeroed, when on
    h->stor_layers = h->stor_bins = 0;
    if (n_layers == 0) return HC_OK;
    if (n_layers < 0 || n_layers > HC_STORAGE_MAX_LAYERS)
        return fail(HC_ERR_ARG, "hc_set_layer_storage: %d layers (1 to %d; 0 = off)", (int)n_layers, HC_STORAGE_MAX_LAYERS);
    if (n_bins != 0 && (n_bins < 32 || n_bins > 1024 || (n_bins & (n_bins - 1))))
        return fail(HC_ERR_ARG, "hc_set_layer_storage: %d bins (a power of two in 32 .. 1024; 0 = no histogram)", (int)n_bins);
    for (int l = 0; l < n_layers; l++) h->stor_range[l][0] = ranges[2 * l], h->stor_range[l][1] = ranges[2 * l + 1];
    h->stor_layers = n_layers, h->stor_bins = n_bins;
    const int rc = ensure_stor(h);           // (its refusals come before anything is allocated)
    if (rc != HC_OK) h->stor_layers = h->stor_bins = 0, h->stor.release(), h->shist.release();      // refused: off
    return rc;
}

int hc_get_layer_storage_words(hc_handle *h, int64_t *n_words)
{
    if (!h || !n_words) return fail(HC_ERR_ARG, "hc_get_layer_storage_words: bad argument");
    if (int rc = ensure_stor(h)) return rc;
    *n_words = h->stor.n;
    return HC_OK;
}

int hc_get_layer_storage(hc_handle *h, int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_layer_storage: bad argument");
    return table_copy(h, h->stor, ensure_stor, hipMemcpyDeviceToHost, table, n_words, "hc_get_layer_storage");
}

int hc_set_layer_storage_tables(hc_handle *h, const int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_layer_storage_tables: bad argument");
    return table_copy(h, h->stor, ensure_stor, hipMemcpyHostToDevice, const_cast<int64_t *>(table), n_words,
                      "hc_set_layer_storage_tables");
}

int hc_export_layer_storage(hc_handle *h, void *device_dst, int64_t n_words)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_layer_storage: bad argument");
    return table_copy(h, h->stor, ensure_stor, hipMemcpyDeviceToDevice, device_dst, n_words, "hc_export_layer_storage");
}

int hc_get_layer_storage_hist(hc_handle *h, int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_layer_storage_hist: bad argument");
    return table_copy(h, h->shist, ensure_stor_hist, hipMemcpyDeviceToHost, table, n_entries, "hc_get_layer_storage_hist");
}

int hc_set_layer_storage_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_layer_storage_hist_table: bad argument");
    return table_copy(h, h->shist, ensure_stor_hist, hipMemcpyHostToDevice, const_cast<int32_t *>(table), n_entries,
                      "hc_set_layer_storage_hist_table");
}

int hc_reset_layer_storage(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_layer_storage: bad argument");
    h->shist.invalidate();
    return table_reset(h, h->stor, ensure_stor);
}

int hc_get_layer_storage_outside(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_layer_storage_outside: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_stor(h)) return rc;
    *count = 0;
    if (h->stor_bins == 0) return HC_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->shist.buf.p + (h->shist.n - 2), 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_layer_storage_overflow(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_layer_storage_overflow: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_stor(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->stor.buf.p + stor_layout(h).ovf, 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_layer_storage_layout(hc_handle *h, int32_t *n_layers, int32_t *n_bins, int32_t *ranges)
{
    if (!h || !n_layers || !n_bins || !ranges) return fail(HC_ERR_ARG, "hc_get_layer_storage_layout: bad argument");
    *n_layers = h->stor_layers, *n_bins = h->stor_bins;
    for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++)
        ranges[2 * l] = l < h->stor_layers ? h->stor_range[l][0] : 0, ranges[2 * l + 1] = l < h->stor_layers ? h->stor_range[l][1] : 0;
    return HC_OK;
}

int hc_set_conductivity_stats(hc_handle *h, int32_t n_layers, const int32_t *ranges)
{
    if (!h || (n_layers > 0 && !ranges)) return fail(HC_ERR_ARG, "hc_set_conductivity_stats: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    cond_off(h);                 // re-created, zeroed, when on
    if (n_layers < 0) return HC_OK;
    if (n_layers > HC_STORAGE_MAX_LAYERS)
        return fail(HC_ERR_ARG, "hc_set_conductivity_stats: %d layers (0 to %d; -1 = off)", (int)n_layers, HC_STORAGE_MAX_LAYERS);
    for (int l = 0; l < n_layers; l++) h->cond_range[l][0] = ranges[2 * l], h->cond_range[l][1] = ranges[2 * l + 1];
    h->cond_on = true, h->cond_layers = n_layers;
    const int rc = ensure_cond(h);           // (its refusals come before anything is allocated)
    if (rc != HC_OK) cond_off(h);            // refused: off
    return rc;
}

int hc_clear_conductivity_stats(hc_handle *h) { return hc_set_conductivity_stats(h, -1, nullptr); }

int hc_get_conductivity_stats_words(hc_handle *h, int64_t *n_words)
{
    if (!h || !n_words) return fail(HC_ERR_ARG, "hc_get_conductivity_stats_words: bad argument");
    if (int rc = ensure_cond(h)) return rc;
    *n_words = h->cond.n;
    return HC_OK;
}

int hc_get_conductivity_stats(hc_handle *h, int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_conductivity_stats: bad argument");
    return table_copy(h, h->cond, ensure_cond, hipMemcpyDeviceToHost, table, n_words, "hc_get_conductivity_stats");
}

int hc_set_conductivity_stats_tables(hc_handle *h, const int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_conductivity_stats_tables: bad argument");
    return table_copy(h, h->cond, ensure_cond, hipMemcpyHostToDevice, const_cast<int64_t *>(table), n_words,
                      "hc_set_conductivity_stats_tables");
}

int hc_export_conductivity_stats(hc_handle *h, void *device_dst, int64_t n_words)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_conductivity_stats: bad argument");
    return table_copy(h, h->cond, ensure_cond, hipMemcpyDeviceToDevice, device_dst, n_words, "hc_export_conductivity_stats");
}

int hc_reset_conductivity_stats(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_conductivity_stats: bad argument");
    return table_reset(h, h->cond, ensure_cond);
}

int hc_get_conductivity_stats_layout(hc_handle *h, int32_t *on, int32_t *n_layers, int32_t *ranges)
{
    if (!h || !on || !n_layers || !ranges) return fail(HC_ERR_ARG, "hc_get_conductivity_stats_layout: bad argument");
    *on = h->cond_on ? 1 : 0, *n_layers = h->cond_layers;
    for (int l = 0; l < HC_STORAGE_MAX_LAYERS; l++)
        ranges[2 * l] = l < h->cond_layers ? h->cond_range[l][0] : 0, ranges[2 * l + 1] = l < h->cond_layers ? h->cond_range[l][1] : 0;
    return HC_OK;
}

int hc_get_conductivity_stats_overflow(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_conductivity_stats_overflow: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_cond(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->cond.buf.p + cond_layout(h).ovf, 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_conductivity_eval(hc_handle *h, int64_t row, double *out)
{
    if (!h || !out) return fail(HC_ERR_ARG, "hc_conductivity_eval: bad argument");
    StepArgs A;
    int rc = fill_args(h, A);
    if (rc) return rc;
    if (row < 0 || row >= h->n_rows) return fail(HC_ERR_ARG, "hc_conductivity_eval: row %lld outside [0, %lld)", (long long)row,
                                                 (long long)h->n_rows);
    HIP_TRY(hipSetDevice(h->device));
    const size_t n = (size_t)h->n_members * h->p.dim_d;
    if (h->scratch_d.ensure(4 * n)) return HC_ERR_DEVICE;
    if ((rc = launch_conductivity(h, A, ProfLayout{}, h->psi.p, row, 0, nullptr, h->scratch_d.p))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->scratch_d.p, 4 * n * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_theta_cov(hc_handle *h, int32_t node_stride)
{
    if (!h) return fail(HC_ERR_ARG, "hc_set_theta_cov: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->cov.release(), h->cov_q.release();    // re-created, zeroed, when on
    h->cov_stride = 0;
    if (node_stride == 0) return HC_OK;
    if (node_stride < 1) return fail(HC_ERR_ARG, "hc_set_theta_cov: node stride %d (>= 1; 0 = off)", (int)node_stride);
    h->cov_stride = node_stride;
    const int rc = ensure_cov(h);            // (its refusals come before anything is allocated)
    if (rc != HC_OK) h->cov_stride = 0, h->cov.release();        // refused: off
    return rc;
}

int hc_get_theta_cov_layout(hc_handle *h, int32_t *node_stride, int32_t *n_nodes, int64_t *words_per_row)
{
    if (!h || !node_stride || !n_nodes || !words_per_row) return fail(HC_ERR_ARG, "hc_get_theta_cov_layout: bad argument");
    *node_stride = *n_nodes = 0, *words_per_row = 0;
    if (h->cov_stride <= 0) return HC_OK;
    const CovLayout C = cov_layout(h);
    *node_stride = C.s, *n_nodes = C.n, *words_per_row = C.W;
    return HC_OK;
}

int hc_get_theta_cov_words(hc_handle *h, int64_t *n_words)
{
    if (!h || !n_words) return fail(HC_ERR_ARG, "hc_get_theta_cov_words: bad argument");
    if (int rc = ensure_cov(h)) return rc;
    *n_words = h->cov.n;
    return HC_OK;
}

int hc_get_theta_cov(hc_handle *h, int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_theta_cov: bad argument");
    return table_copy(h, h->cov, ensure_cov, hipMemcpyDeviceToHost, table, n_words, "hc_get_theta_cov");
}

int hc_set_theta_cov_tables(hc_handle *h, const int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_theta_cov_tables: bad argument");
    return table_copy(h, h->cov, ensure_cov, hipMemcpyHostToDevice, const_cast<int64_t *>(table), n_words,
                      "hc_set_theta_cov_tables");
}

int hc_export_theta_cov(hc_handle *h, void *device_dst, int64_t n_words)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_theta_cov: bad argument");
    return table_copy(h, h->cov, ensure_cov, hipMemcpyDeviceToDevice, device_dst, n_words, "hc_export_theta_cov");
}

int hc_reset_theta_cov(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_theta_cov: bad argument");
    return table_reset(h, h->cov, ensure_cov);
}

int hc_get_theta_cov_outside(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_theta_cov_outside: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_cov(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->cov.buf.p + (h->cov.n - 1), 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

void period_off(hc_handle *h)
{
    h->per_n = h->per_nthr = h->per_bins = 0;
    h->per_end.clear();
    h->pacc.release(), h->pacc_alt.release(), h->pmom.release(), h->phist.release();
}

int hc_set_period_totals(hc_handle *h, int32_t n_periods, const int64_t *end_rows, int32_t n_thresholds,
                         const int32_t *threshold_nodes, int32_t n_bins, const int32_t *flux_max_log2)
{
    if (!h || (n_periods > 0 && !end_rows) || (n_periods > 0 && n_thresholds > 0 && !threshold_nodes))
        return fail(HC_ERR_ARG, "hc_set_period_totals: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    // the root uptake (hc_set_root_uptake) lives on these periods: other ends turn it off, the same ends re-create its
    // tables and accumulators, zeroed, with the period totals'
    const bool same_ends = n_periods > 0 && (size_t)n_periods == h->per_end.size() &&
                           std::equal(h->per_end.begin(), h->per_end.end(), end_rows);
    const int keep_layers = same_ends ? h->upt_layers : 0, keep_bins = h->upt_bins;      // (the ranges stay where they are)
    uptake_off(h);
    period_off(h);               // the tables and the accumulators are re-created when on
    if (n_periods == 0) return HC_OK;
    if (n_periods < 0 || n_periods > HC_PERIOD_MAX_PERIODS)
        return fail(HC_ERR_ARG, "hc_set_period_totals: %d periods (1 to %d; 0 = off)", (int)n_periods, HC_PERIOD_MAX_PERIODS);
    for (int p = 0; p < n_periods; p++) {
        const int64_t prev = p > 0 ? end_rows[p - 1] : 0;
        if (end_rows[p] < 1 || end_rows[p] >= h->n_rows || end_rows[p] <= prev)
            return fail(HC_ERR_ARG, "hc_set_period_totals: end row %lld of period %d (ascending rows in [1, %lld))",
                        (long long)end_rows[p], p, (long long)h->n_rows);
        if (end_rows[p] - prev > HC_PERIOD_MAX_ROWS)
            return fail(HC_ERR_ARG, "hc_set_period_totals: period %d holds %lld rows (at most %d)", p,
                        (long long)(end_rows[p] - prev), HC_PERIOD_MAX_ROWS);
    }
    if (n_thresholds < 0 || n_thresholds > HC_PERIOD_MAX_THRESHOLDS)
        return fail(HC_ERR_ARG, "hc_set_period_totals: %d thresholds (0 to %d)", (int)n_thresholds, HC_PERIOD_MAX_THRESHOLDS);
    if (n_bins != 0 && (n_bins < 32 || n_bins > 1024 || (n_bins & (n_bins - 1))))
        return fail(HC_ERR_ARG, "hc_set_period_totals: %d bins (a power of two in 32 .. 1024; 0 = no histograms)", (int)n_bins);
    if (n_bins != 0 && !flux_max_log2) return fail(HC_ERR_ARG, "hc_set_period_totals: histograms need flux_max_log2");
    for (int q = 0; q < 2 && n_bins != 0; q++)
        if (flux_max_log2[q] < -8 || flux_max_log2[q] > 12)
            return fail(HC_ERR_ARG, "hc_set_period_totals: flux_max_log2[%d] = %d (-8 .. 12: 2^e cm)", q, (int)flux_max_log2[q]);
    h->per_end.assign(end_rows, end_rows + n_periods);
    for (int j = 0; j < n_thresholds; j++) h->per_thr[j] = threshold_nodes[j];
    for (int q = 0; q < 2; q++) h->per_fexp[q] = n_bins != 0 ? flux_max_log2[q] : 0;
    h->per_n = n_periods, h->per_nthr = n_thresholds, h->per_bins = n_bins;
    const int rc = ensure_period(h);         // (its refusals come before anything is allocated)
    if (rc != HC_OK) period_off(h);          // refused: off
    if (rc == HC_OK && keep_layers > 0) {
        h->upt_layers = keep_layers, h->upt_bins = keep_bins;
        if (ensure_uptake(h) != HC_OK) uptake_off(h);
    }
    return rc;
}

int hc_get_period_totals_words(hc_handle *h, int64_t *n_words)
{
    if (!h || !n_words) return fail(HC_ERR_ARG, "hc_get_period_totals_words: bad argument");
    if (int rc = ensure_period(h)) return rc;
    *n_words = h->pmom.n;
    return HC_OK;
}

int hc_get_period_totals(hc_handle *h, int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_period_totals: bad argument");
    return table_copy(h, h->pmom, ensure_period, hipMemcpyDeviceToHost, table, n_words, "hc_get_period_totals");
}

int hc_set_period_totals_tables(hc_handle *h, const int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_period_totals_tables: bad argument");
    return table_copy(h, h->pmom, ensure_period, hipMemcpyHostToDevice, const_cast<int64_t *>(table), n_words,
                      "hc_set_period_totals_tables");
}

int hc_export_period_totals(hc_handle *h, void *device_dst, int64_t n_words)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_period_totals: bad argument");
    return table_copy(h, h->pmom, ensure_period, hipMemcpyDeviceToDevice, device_dst, n_words, "hc_export_period_totals");
}

int hc_get_period_totals_hist(hc_handle *h, int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_period_totals_hist: bad argument");
    return table_copy(h, h->phist, ensure_period_hist, hipMemcpyDeviceToHost, table, n_entries, "hc_get_period_totals_hist");
}

int hc_set_period_totals_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_period_totals_hist_table: bad argument");
    return table_copy(h, h->phist, ensure_period_hist, hipMemcpyHostToDevice, const_cast<int32_t *>(table), n_entries,
                      "hc_set_period_totals_hist_table");
}

int hc_export_period_totals_hist(hc_handle *h, void *device_dst, int64_t n_entries)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_period_totals_hist: bad argument");
    return table_copy(h, h->phist, ensure_period_hist, hipMemcpyDeviceToDevice, device_dst, n_entries,
                      "hc_export_period_totals_hist");
}

int hc_get_period_totals_acc(hc_handle *h, int64_t *acc, int64_t n_words)
{
    if (!h || !acc) return fail(HC_ERR_ARG, "hc_get_period_totals_acc: bad argument");
    return table_copy(h, h->pacc, ensure_period_acc, hipMemcpyDeviceToHost, acc, n_words, "hc_get_period_totals_acc");
}

int hc_set_period_totals_acc(hc_handle *h, const int64_t *acc, int64_t n_words)
{
    if (!h || !acc) return fail(HC_ERR_ARG, "hc_set_period_totals_acc: bad argument");
    return table_copy(h, h->pacc, ensure_period_acc, hipMemcpyHostToDevice, const_cast<int64_t *>(acc), n_words,
                      "hc_set_period_totals_acc");
}

int hc_reset_period_totals(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_period_totals: bad argument");
    h->phist.invalidate(), h->pacc.invalidate();
    return table_reset(h, h->pmom, ensure_period);
}

int hc_get_period_totals_outside(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_period_totals_outside: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_period(h)) return rc;
    *count = 0;
    if (h->per_bins == 0) return HC_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->phist.buf.p + (h->phist.n - 2), 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_period_totals_overflow(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_period_totals_overflow: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_period(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->pmom.buf.p + period_layout(h).ovf, 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_period_totals_layout(hc_handle *h, int32_t *n_periods, int32_t *n_thresholds, int32_t *n_bins,
                                int32_t *threshold_nodes, int32_t *flux_max_log2, int64_t *end_rows, int64_t n_end_rows)
{
    if (!h || !n_periods || !n_thresholds || !n_bins || !threshold_nodes || !flux_max_log2)
        return fail(HC_ERR_ARG, "hc_get_period_totals_layout: bad argument");
    *n_periods = h->per_n, *n_thresholds = h->per_nthr, *n_bins = h->per_bins;
    for (int j = 0; j < HC_PERIOD_MAX_THRESHOLDS; j++) threshold_nodes[j] = j < h->per_nthr ? h->per_thr[j] : 0;
    for (int q = 0; q < 2; q++) flux_max_log2[q] = h->per_fexp[q];
    if (end_rows)
        for (int64_t p = 0; p < std::min<int64_t>(n_end_rows, h->per_n); p++) end_rows[p] = h->per_end[(size_t)p];
    return HC_OK;
}

int hc_set_root_uptake(hc_handle *h, int32_t n_layers, const int32_t *cell_lo, const int32_t *cell_hi, int32_t n_bins)
{
    if (!h || (n_layers > 0 && (!cell_lo || !cell_hi))) return fail(HC_ERR_ARG, "hc_set_root_uptake: bad argument");
    if (!h->have_forcing || !h->have_column) return fail(HC_ERR_ARG, "hc_set_column and hc_set_forcing must come first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    uptake_off(h);               // the tables and the accumulators are re-created when on
    if (n_layers == 0) return HC_OK;
    if (h->per_n <= 0) return fail(HC_ERR_ARG, "hc_set_root_uptake: the period totals are off (hc_set_period_totals comes first)");
    if (n_layers < 0 || n_layers > HC_UPTAKE_MAX_LAYERS)
        return fail(HC_ERR_ARG, "hc_set_root_uptake: %d layers (1 to %d; 0 = off)", (int)n_layers, HC_UPTAKE_MAX_LAYERS);
    if (n_bins != 0 && (n_bins < 32 || n_bins > 1024 || (n_bins & (n_bins - 1))))
        return fail(HC_ERR_ARG, "hc_set_root_uptake: %d bins (a power of two in 32 .. 1024; 0 = no histogram)", (int)n_bins);
    if (h->fs_n > 0)
        return fail(HC_ERR_ARG, "hc_set_root_uptake: a sharded particle filter is set (hc_set_filter_shard), and the routed "
                                "columns do not carry the members' accumulators");
    for (int l = 0; l < n_layers; l++) h->upt_range[l][0] = cell_lo[l], h->upt_range[l][1] = cell_hi[l];
    h->upt_layers = n_layers, h->upt_bins = n_bins;
    const int rc = ensure_uptake(h);         // (its refusals come before anything is allocated)
    if (rc != HC_OK) uptake_off(h);          // refused: off
    return rc;
}

int hc_get_root_uptake_words(hc_handle *h, int64_t *n_words)
{
    if (!h || !n_words) return fail(HC_ERR_ARG, "hc_get_root_uptake_words: bad argument");
    if (int rc = ensure_uptake(h)) return rc;
    *n_words = h->upt.n;
    return HC_OK;
}

int hc_get_root_uptake(hc_handle *h, int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_root_uptake: bad argument");
    return table_copy(h, h->upt, ensure_uptake, hipMemcpyDeviceToHost, table, n_words, "hc_get_root_uptake");
}

int hc_set_root_uptake_tables(hc_handle *h, const int64_t *table, int64_t n_words)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_root_uptake_tables: bad argument");
    return table_copy(h, h->upt, ensure_uptake, hipMemcpyHostToDevice, const_cast<int64_t *>(table), n_words,
                      "hc_set_root_uptake_tables");
}

int hc_export_root_uptake(hc_handle *h, void *device_dst, int64_t n_words)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_root_uptake: bad argument");
    return table_copy(h, h->upt, ensure_uptake, hipMemcpyDeviceToDevice, device_dst, n_words, "hc_export_root_uptake");
}

int hc_get_root_uptake_hist(hc_handle *h, int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_root_uptake_hist: bad argument");
    return table_copy(h, h->uhist, ensure_uptake_hist, hipMemcpyDeviceToHost, table, n_entries, "hc_get_root_uptake_hist");
}

int hc_set_root_uptake_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_root_uptake_hist_table: bad argument");
    return table_copy(h, h->uhist, ensure_uptake_hist, hipMemcpyHostToDevice, const_cast<int32_t *>(table), n_entries,
                      "hc_set_root_uptake_hist_table");
}

int hc_export_root_uptake_hist(hc_handle *h, void *device_dst, int64_t n_entries)
{
    if (!h || !device_dst) return fail(HC_ERR_ARG, "hc_export_root_uptake_hist: bad argument");
    return table_copy(h, h->uhist, ensure_uptake_hist, hipMemcpyDeviceToDevice, device_dst, n_entries,
                      "hc_export_root_uptake_hist");
}

int hc_get_root_uptake_acc(hc_handle *h, int64_t *acc, int64_t n_words)
{
    if (!h || !acc) return fail(HC_ERR_ARG, "hc_get_root_uptake_acc: bad argument");
    return table_copy(h, h->uacc, ensure_uptake_acc, hipMemcpyDeviceToHost, acc, n_words, "hc_get_root_uptake_acc");
}

int hc_set_root_uptake_acc(hc_handle *h, const int64_t *acc, int64_t n_words)
{
    if (!h || !acc) return fail(HC_ERR_ARG, "hc_set_root_uptake_acc: bad argument");
    return table_copy(h, h->uacc, ensure_uptake_acc, hipMemcpyHostToDevice, const_cast<int64_t *>(acc), n_words,
                      "hc_set_root_uptake_acc");
}

int hc_reset_root_uptake(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_root_uptake: bad argument");
    h->uhist.invalidate(), h->uacc.invalidate();
    return table_reset(h, h->upt, ensure_uptake);
}

int hc_get_root_uptake_outside(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_root_uptake_outside: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_uptake(h)) return rc;
    *count = 0;
    if (h->upt_bins == 0) return HC_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->uhist.buf.p + (h->uhist.n - 2), 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_root_uptake_overflow(hc_handle *h, uint64_t *count)
{
    if (!h || !count) return fail(HC_ERR_ARG, "hc_get_root_uptake_overflow: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_uptake(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(count, h->upt.buf.p + uptake_layout(h).ovf, 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_root_uptake_layout(hc_handle *h, int32_t *n_layers, int32_t *n_bins, int32_t *cell_lo, int32_t *cell_hi)
{
    if (!h || !n_layers || !n_bins || !cell_lo || !cell_hi) return fail(HC_ERR_ARG, "hc_get_root_uptake_layout: bad argument");
    *n_layers = h->upt_layers, *n_bins = h->upt_bins;
    for (int l = 0; l < HC_UPTAKE_MAX_LAYERS; l++) {
        cell_lo[l] = l < h->upt_layers ? h->upt_range[l][0] : 0;
        cell_hi[l] = l < h->upt_layers ? h->upt_range[l][1] : 0;
    }
    return HC_OK;
}

int hc_root_uptake_eval(hc_handle *h, int64_t row, double *theta_mid, double *u)
{
    if (!h || !theta_mid || !u) return fail(HC_ERR_ARG, "hc_root_uptake_eval: bad argument");
    StepArgs A;
    int rc = fill_args(h, A);
    if (rc) return rc;
    if (row < 0 || row >= h->n_rows) return fail(HC_ERR_ARG, "hc_root_uptake_eval: row %lld outside [0, %lld)", (long long)row,
                                                 (long long)h->n_rows);
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = ensure_mid_tabs(h))) return rc;
    const size_t n = (size_t)h->n_members * (h->p.dim_d - 1);
    if (h->scratch_d.ensure(2 * n)) return HC_ERR_DEVICE;
    if ((rc = launch_root_uptake(h, A, h->psi.p, row, 1, h->scratch_d.p, h->scratch_d.p + n))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(theta_mid, h->scratch_d.p, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(u, h->scratch_d.p + n, n * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_wtd_distribution(int device, const int32_t *hist, const int32_t *obs_idx, int64_t n_rows, int32_t D,
                        const double *levels, int32_t n_levels, double dz, int64_t *count, int32_t *quantile_idx,
                        double *crps_cm)
{
    if (device < 0 || n_rows < 0 || D < 2 || D > HC_MAX_DEPTH_NODES || n_levels < 0 || n_levels > HC_WTD_MAX_LEVELS ||
        !std::isfinite(dz))
        return fail(HC_ERR_ARG, "hc_wtd_distribution: bad argument (D = %d in [2, %d], %d levels of at most %d)", (int)D,
                    HC_MAX_DEPTH_NODES, (int)n_levels, HC_WTD_MAX_LEVELS);
    if (n_rows > HC_WTD_HIST_MAX_ENTRIES / D)
        return fail(HC_ERR_ARG, "hc_wtd_distribution: %lld rows of %d bins exceed HC_WTD_HIST_MAX_ENTRIES", (long long)n_rows, (int)D);
    if (n_rows > 0 && (!hist || !obs_idx || !count || !crps_cm || (n_levels > 0 && (!levels || !quantile_idx))))
        return fail(HC_ERR_ARG, "hc_wtd_distribution: NULL argument");
    WtdLevels lv{};
    for (int l = 0; l < n_levels; l++) {
        if (!(levels[l] >= 0.0 && levels[l] <= 1.0))
            return fail(HC_ERR_ARG, "hc_wtd_distribution: level %d = %g is outside [0, 1]", l, levels[l]);
        lv.q[l] = levels[l];
    }
    if (n_rows == 0) return HC_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf<int> d_hist, d_obs, d_q;
    DevBuf<long long> d_count;
    DevBuf<double> d_crps;
    const int rc = wtd_distribution_run(hist, obs_idx, n_rows, D, lv, n_levels, dz, count, quantile_idx, crps_cm, d_hist,
                                        d_obs, d_count, d_q, d_crps);
    d_hist.release(); d_obs.release(); d_q.release(); d_count.release(); d_crps.release();
    return rc;
}

int hc_set_filter(hc_handle *h, int32_t stride, double sigma_cm, uint64_t seed)
{
    if (!h || stride < 0) return fail(HC_ERR_ARG, "hc_set_filter: bad argument");
    if (stride > 0 && h->enkf_stride > 0)
        return fail(HC_ERR_ARG, "hc_set_filter: the EnKF is on (hc_set_enkf with stride 0 turns it off)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    filter_off(h);
    if (stride == 0) return HC_OK;
    if (!(std::isfinite(sigma_cm) && sigma_cm > 0.0))
        return fail(HC_ERR_ARG, "hc_set_filter: sigma_cm = %g must be finite and > 0", sigma_cm);
    StepArgs A;
    if (int rc = fill_args(h, A)) return rc;     // column, forcing, members and noise are in place; point keys uploaded
    if (h->n_rows > (int64_t)UINT32_MAX) return fail(HC_ERR_ARG, "hc_set_filter: %lld forcing rows exceed 2^32 - 1", (long long)h->n_rows);
    if (A.members_per_point > INT32_MAX)
        return fail(HC_ERR_ARG, "hc_set_filter: %lld members per point exceed 2^31 - 1", (long long)A.members_per_point);
    h->filt_stride = stride;
    h->filt_sigma = sigma_cm;
    h->filt_seed = seed;
    int rc = ensure_filter(h);
    if (rc == HC_OK && h->philox && !h->ncorr) {
        // the base vectors the kernel's Philox path would build, z * scale (one rounding), from here on carried like
        // the caller's: damped in place, copied from the ancestor (a correlated source's are in place already)
        const size_t total = (size_t)h->n_members * h->p.dim_d;
        rc = h->base.ensure(total);
        if (rc == HC_OK) rc = launch_noise_fill(h, h->base.p, 1, nullptr, h->nscale.p);
        if (rc == HC_OK) {
            const hipError_t e = hipGetLastError();
            const hipError_t e2 = hipStreamSynchronize(h->stream);
            if (e != hipSuccess || e2 != hipSuccess)
                rc = fail(HC_ERR_DEVICE, "hc_set_filter: base vectors: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        }
    }
    if (rc != HC_OK) filter_off(h);              // refused: off
    return rc;
}

int hc_get_filter_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_filter_stats: bad argument");
    return table_copy(h, h->filt, ensure_filter, hipMemcpyDeviceToHost, table, n_entries, "hc_get_filter_stats");
}

int hc_set_filter_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_filter_stats: bad argument");
    return table_copy(h, h->filt, ensure_filter, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_filter_stats");
}

// the last assimilation's buffers (test hooks): a device -> host copy of `count` entries
}  // extern "C"
namespace {
// what a soil-moisture record must satisfy, the EnKF's and the particle filter's alike: nodes in the column, sigma finite
// and > 0, values in [0, 1] or NaN
int sm_record_check(const hc_handle *h, const char *who, int32_t n_sensors, const int32_t *nodes, const double *values,
                           const double *sigma)
{
    const int D = h->p.dim_d;
    for (int i = 0; i < n_sensors; i++) {
        if (nodes[i] < 0 || nodes[i] >= D)
            return fail(HC_ERR_ARG, "%s: node %d of sensor %d outside [0, %d)", who, (int)nodes[i], i, D);
        if (!(std::isfinite(sigma[i]) && sigma[i] > 0.0))
            return fail(HC_ERR_ARG, "%s: sigma %g of sensor %d must be finite and > 0", who, sigma[i], i);
    }
    const size_t n = (size_t)h->n_rows * n_sensors;
    for (size_t k = 0; k < n; k++)
        if (!std::isnan(values[k]) && !(values[k] >= 0.0 && values[k] <= 1.0))
            return fail(HC_ERR_ARG, "%s: value %g (row %lld, sensor %d) outside [0, 1]", who, values[k],
                        (long long)(k / n_sensors), (int)(k % n_sensors));
    return HC_OK;
}

// The bodies hc_set_filter_soil_moisture and hc_set_enkf_soil_moisture share, after the owner's own refusals: the
// arguments, against the owner's window of `n_window` offsets too; the stream drained; the record cleared by the owner's
// `off` (with what else the owner releases) and, with sensors, stored, its table made by the owner's `ensure`
int record_set(hc_handle *h, SmRecord &r, int n_window, void (*off)(hc_handle *), int (*ensure)(hc_handle *),
               const char *who, int32_t n_sensors, const int32_t *nodes, const double *values, const double *sigma)
{
    if (n_sensors > 0 && (!nodes || !values || !sigma)) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (n_sensors + n_window > ENKF_SENSORS)
        return fail(HC_ERR_ARG, "%s: %d sensors and %d window offsets, at most %d together", who, (int)n_sensors, n_window,
                    ENKF_SENSORS);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    off(h);
    if (n_sensors == 0) return HC_OK;
    if (int rc = sm_record_check(h, who, n_sensors, nodes, values, sigma)) return rc;
    r.nodes.assign(nodes, nodes + n_sensors);
    r.sigma.assign(sigma, sigma + n_sensors);
    r.values.assign(values, values + (size_t)h->n_rows * n_sensors);
    r.rows = h->n_rows;
    r.n = n_sensors;
    const int rc = ensure(h);
    if (rc != HC_OK) off(h);                     // refused: off
    return rc;
}

// ... and hc_set_filter_window and hc_set_enkf_window: the offsets against the owner's record of `n_sensors` sensors and
// its stride, sorted; then as above
int window_set(hc_handle *h, WindowBase &w, int n_sensors, int stride, void (*off)(hc_handle *), int (*ensure)(hc_handle *),
               const char *who, int32_t n_offsets, const int32_t *offsets)
{
    if (n_offsets + n_sensors > ENKF_SENSORS)
        return fail(HC_ERR_ARG, "%s: %d offsets and %d sensors, at most %d together", who, (int)n_offsets, n_sensors,
                    ENKF_SENSORS);
    std::vector<int> sorted(offsets, offsets + n_offsets);
    std::sort(sorted.begin(), sorted.end());
    for (int j = 0; j < n_offsets; j++) {
        if (sorted[(size_t)j] < 1 || sorted[(size_t)j] >= stride)
            return fail(HC_ERR_ARG, "%s: offset %d outside [1, %d) (the stride)", who, sorted[(size_t)j], stride);
        if (j > 0 && sorted[(size_t)j] == sorted[(size_t)j - 1])
            return fail(HC_ERR_ARG, "%s: offset %d twice", who, sorted[(size_t)j]);
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    off(h);
    if (n_offsets == 0) return HC_OK;
    w.n = n_offsets;
    w.off = sorted;
    w.row.assign((size_t)n_offsets, (int64_t)-1);
    const int rc = ensure(h);
    if (rc != HC_OK) off(h);                     // refused: off
    return rc;
}

// What a window holds for the coming assimilation (checkpoints): out, an empty slot as zeros; the checks of what comes
// in (`setter`: the entry point that sets the window); in
template <typename T>
int window_capture_get(hc_handle *h, const Window<T> &w, const char *who, const char *setter, T *cap, int64_t *rows)
{
    if (w.n <= 0) return fail(HC_ERR_ARG, "%s: no window offsets (%s)", who, setter);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->n_members;
    for (int j = 0; j < w.n; j++) {
        rows[j] = w.row[(size_t)j];
        if (rows[j] >= 0)
            HIP_TRY(hipMemcpy(cap + (size_t)j * N, w.cap.p + (size_t)j * N, N * sizeof(T), hipMemcpyDeviceToHost));
        else
            std::fill_n(cap + (size_t)j * N, N, T(0));
    }
    return HC_OK;
}
int window_capture_check(const hc_handle *h, const WindowBase &w, const char *who, const char *setter, const int64_t *rows)
{
    if (w.n <= 0) return fail(HC_ERR_ARG, "%s: no window offsets (%s)", who, setter);
    for (int j = 0; j < w.n; j++)
        if (rows[j] < -1 || rows[j] >= h->n_rows)
            return fail(HC_ERR_ARG, "%s: row %lld of offset %d outside [-1, %lld)", who, (long long)rows[j], w.off[(size_t)j],
                        (long long)h->n_rows);
    return HC_OK;
}
template <typename T>
int window_capture_set(hc_handle *h, Window<T> &w, const T *cap, const int64_t *rows)
{
    const size_t n = (size_t)w.n * h->n_members;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (w.cap.ensure(n)) return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpy(w.cap.p, cap, n * sizeof(T), hipMemcpyHostToDevice));
    w.row.assign(rows, rows + w.n);
    return HC_OK;
}

// the lagged columns of the owner's last assimilation (`done`: it is on and one has run), their slots in column order
int window_width(const WindowBase &w, bool done, int32_t *width, int32_t *slots)
{
    *width = done && w.n > 0 ? (int32_t)w.last.size() : 0;
    if (slots)
        for (int k = 0; k < *width; k++) slots[k] = w.last[(size_t)k];
    return HC_OK;
}

template <typename T>
int filter_hook(hc_handle *h, const DevBuf<T> &b, void *out, size_t count, const char *who, size_t first = 0)
{
    if (!h || !out) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (h->filt_stride <= 0 || !h->filt_done) return fail(HC_ERR_ARG, "%s: no assimilation since hc_set_filter", who);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, b.p + first, count * sizeof(T), hipMemcpyDeviceToHost));
    return HC_OK;
}
}  // namespace
extern "C" {

int hc_get_filter_ancestors(hc_handle *h, int64_t *ancestors)
{
    // (hc_set_filter_shard: the table is the whole point's, in global ids; the handle's own slots of it)
    const size_t first = h && h->fs_n > 0 ? (size_t)h->fs_bounds[(size_t)h->fs_index] : 0;
    return filter_hook(h, h->filt_anc, ancestors, h ? (size_t)h->n_members : 0, "hc_get_filter_ancestors", first);
}

int hc_get_filter_weights(hc_handle *h, int64_t *q)
{
    return filter_hook(h, h->filt_q, q, (size_t)h->n_points * h->p.dim_d, "hc_get_filter_weights");
}

int hc_get_filter_draw(hc_handle *h, int64_t *r)
{
    if (!h || !r) return fail(HC_ERR_ARG, "hc_get_filter_draw: bad argument");
    std::vector<unsigned long long> qr((size_t)2 * h->n_points);
    if (int rc = filter_hook(h, h->filt_qr, qr.data(), qr.size(), "hc_get_filter_draw")) return rc;
    for (int p = 0; p < h->n_points; p++) r[p] = (int64_t)qr[(size_t)2 * p + 1];
    return HC_OK;
}

int hc_get_filter_base(hc_handle *h, double *base, int64_t first, int64_t count)
{
    if (!h || !base || first < 0 || count < 0 || first + count > h->n_members || !h->filt_host())
        return fail(HC_ERR_ARG, "hc_get_filter_base: bad argument (a Philox run with the particle filter on)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int D = h->p.dim_d;
    HIP_TRY(hipMemcpy(base, h->base.p + (size_t)first * D, (size_t)count * D * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_filter_base(hc_handle *h, const double *base)
{
    if (!h || !base || !h->filt_host())
        return fail(HC_ERR_ARG, "hc_set_filter_base: bad argument (a Philox run with the particle filter on)");
    const size_t n = (size_t)h->n_members * h->p.dim_d;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(base[i])) return fail(HC_ERR_ARG, "hc_set_filter_base: entry %zu is not finite", i);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->base.p, base, n * 8, hipMemcpyHostToDevice));
    return HC_OK;
}

int hc_set_filter_soil_moisture(hc_handle *h, int32_t n_sensors, const int32_t *nodes, const double *values,
                                const double *sigma)
{
    if (!h || n_sensors < 0) return fail(HC_ERR_ARG, "hc_set_filter_soil_moisture: bad argument");
    if (n_sensors > ENKF_SENSORS)
        return fail(HC_ERR_ARG, "hc_set_filter_soil_moisture: %d sensors, at most %d", (int)n_sensors, ENKF_SENSORS);
    if (n_sensors > 0 && h->enkf_stride > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_soil_moisture: the EnKF is on (its record: hc_set_enkf_soil_moisture)");
    if (n_sensors > 0 && h->filt_stride <= 0)
        return fail(HC_ERR_ARG, "hc_set_filter_soil_moisture: the particle filter is off (hc_set_filter comes first)");
    if (n_sensors > 0 && h->fs_n > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_soil_moisture: the filter is sharded (hc_set_filter_shard), and the sharded "
                                "filter gathers water-table indices only: a record needs every member of a point on one handle");
    return record_set(h, h->filt_sm, h->filt_win.n, fsm_off, ensure_fsm, "hc_set_filter_soil_moisture", n_sensors, nodes,
                      values, sigma);
}

int hc_get_filter_sm_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_filter_sm_stats: bad argument");
    return table_copy(h, h->filt_sm.table, ensure_fsm, hipMemcpyDeviceToHost, table, n_entries, "hc_get_filter_sm_stats");
}

int hc_set_filter_sm_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_filter_sm_stats: bad argument");
    return table_copy(h, h->filt_sm.table, ensure_fsm, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_filter_sm_stats");
}

int hc_set_filter_tempering(hc_handle *h, double ess_floor)
{
    if (!h) return fail(HC_ERR_ARG, "hc_set_filter_tempering: bad argument");
    if (ess_floor != 0.0 && !(std::isfinite(ess_floor) && ess_floor > 0.0 && ess_floor < 1.0))
        return fail(HC_ERR_ARG, "hc_set_filter_tempering: ess_floor = %g must be 0 (off) or finite with 0 < f < 1", ess_floor);
    if (ess_floor != 0.0 && h->filt_stride <= 0)
        return fail(HC_ERR_ARG, "hc_set_filter_tempering: the particle filter is off (hc_set_filter comes first)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    temper_off(h);
    if (ess_floor == 0.0) return HC_OK;
    h->filt_floor = ess_floor;
    const int rc = ensure_ftemp(h);
    if (rc != HC_OK) temper_off(h);              // refused: off
    return rc;
}

int hc_get_filter_temper_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_filter_temper_stats: bad argument");
    return table_copy(h, h->ftemp, ensure_ftemp, hipMemcpyDeviceToHost, table, n_entries, "hc_get_filter_temper_stats");
}

int hc_set_filter_temper_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_filter_temper_stats: bad argument");
    return table_copy(h, h->ftemp, ensure_ftemp, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_filter_temper_stats");
}

int hc_get_filter_temper_trials(hc_handle *h, int64_t *trials)
{
    if (h && h->filt_floor <= 0.0) return fail(HC_ERR_ARG, "hc_get_filter_temper_trials: the weights are not tempered");
    return filter_hook(h, h->filt_trials, trials, h ? (size_t)h->n_points * TEMPER_TRIALS * TEMPER_WIDTH : 0,
                       "hc_get_filter_temper_trials");
}

int hc_set_filter_rejuvenation(hc_handle *h, double discount)
{
    if (!h) return fail(HC_ERR_ARG, "hc_set_filter_rejuvenation: bad argument");
    if (discount != 0.0 && !(std::isfinite(discount) && discount >= 0.5 && discount < 1.0))
        return fail(HC_ERR_ARG, "hc_set_filter_rejuvenation: discount = %g must be 0 (off) or finite with 0.5 <= discount < 1",
                    discount);
    if (discount != 0.0 && h->filt_stride <= 0)
        return fail(HC_ERR_ARG, "hc_set_filter_rejuvenation: the particle filter is off (hc_set_filter comes first)");
    if (discount != 0.0 && h->fs_n > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_rejuvenation: the filter is sharded (hc_set_filter_shard), and the sharded "
                                "filter gathers water-table indices only: the moments of the base vectors would need an "
                                "exchange of their own");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    rejuv_off(h);
    if (discount == 0.0) return HC_OK;
    // Liu & West's shrinkage, every operation rounded once
    const double a = (3.0 * discount - 1.0) / (2.0 * discount);
    h->rj_delta = discount;
    h->rj_a = a;
    h->rj_h = std::sqrt(1.0 - a * a);
    const int rc = ensure_frej(h);
    if (rc != HC_OK) rejuv_off(h);               // refused: off
    return rc;
}

int hc_get_filter_rejuvenation(hc_handle *h, double *discount, double *shrinkage)
{
    if (!h || !discount || !shrinkage) return fail(HC_ERR_ARG, "hc_get_filter_rejuvenation: bad argument");
    *discount = h->rj_delta;
    *shrinkage = h->rj_delta > 0.0 ? h->rj_a : 0.0;
    return HC_OK;
}

int hc_get_filter_rejuvenation_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_filter_rejuvenation_stats: bad argument");
    return table_copy(h, h->frej, ensure_frej, hipMemcpyDeviceToHost, table, n_entries, "hc_get_filter_rejuvenation_stats");
}

int hc_set_filter_rejuvenation_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_filter_rejuvenation_stats: bad argument");
    return table_copy(h, h->frej, ensure_frej, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_filter_rejuvenation_stats");
}

int hc_get_filter_rejuvenation_moments(hc_handle *h, double *moments)
{
    if (!h || !moments) return fail(HC_ERR_ARG, "hc_get_filter_rejuvenation_moments: bad argument");
    if (h->rj_delta <= 0.0)
        return fail(HC_ERR_ARG, "hc_get_filter_rejuvenation_moments: the base vectors are not rejuvenated");
    if (!h->rj_mom.p) return fail(HC_ERR_ARG, "hc_get_filter_rejuvenation_moments: no assimilation since the setting");
    return filter_hook(h, h->rj_mom, moments, (size_t)h->n_points * 3 * h->p.dim_d, "hc_get_filter_rejuvenation_moments");
}

int hc_filter_rejuvenation_normals(hc_handle *h, int64_t row, int64_t first_member, int64_t count, double *out)
{
    if (!h || !out || row < 0 || row > (int64_t)UINT32_MAX || first_member < 0 || count < 0 ||
        first_member + count > h->n_members)
        return fail(HC_ERR_ARG, "hc_filter_rejuvenation_normals: bad argument");
    if (h->filt_stride <= 0) return fail(HC_ERR_ARG, "hc_filter_rejuvenation_normals: the particle filter is off (hc_set_filter)");
    // the points' keys: hc_set_filter uploaded them (fill_args), and new keys or a new member offset turn the filter off
    if (h->n_points > 1 && !h->point_base.p)
        return fail(HC_ERR_ARG, "hc_filter_rejuvenation_normals: the points' member bases are not in place (hc_set_filter)");
    if (count == 0) return HC_OK;
    HIP_TRY(hipSetDevice(h->device));
    const int D = h->p.dim_d;
    const size_t n = (size_t)count * D;
    DevBuf<double> eps;
    if (eps.ensure(n)) return HC_ERR_DEVICE;
    const long long work = (long long)count * ((D + 1) / 2);
    hipLaunchKernelGGL(filter_rejuv_normals_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, h->stream,
                       (unsigned long long)h->filt_seed, h->n_points > 1 ? h->point_base.p : nullptr,
                       (long long)h->member_offset, (long long)(h->n_members / h->n_points), (unsigned)row,
                       (long long)first_member, (long long)count, D, eps.p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(out, eps.p, n * 8, hipMemcpyDeviceToHost);
    eps.release();
    if (e != hipSuccess) return fail(HC_ERR_DEVICE, "hc_filter_rejuvenation_normals: %s", hipGetErrorString(e));
    return HC_OK;
}

int hc_get_filter_sm_width(hc_handle *h, int32_t *width)
{
    if (!h || !width) return fail(HC_ERR_ARG, "hc_get_filter_sm_width: bad argument");
    *width = h->filt_sm.n > 0 ? h->filt_sm.width : 0;
    return HC_OK;
}

int hc_get_filter_member_weights(hc_handle *h, int64_t *q)
{
    if (h && h->filt_sm.n <= 0 && h->filt_win.n <= 0)
        return fail(HC_ERR_ARG, "hc_get_filter_member_weights: no soil-moisture record");
    return filter_hook(h, h->filt_qm, q, h ? (size_t)h->n_members : 0, "hc_get_filter_member_weights");
}

// columns [col0, col0 + cols) of the last per-member row's Y [N][m_s + m_w + 2]
static int filter_sm_hook(hc_handle *h, double *out, int col0, int cols, const char *who)
{
    if (!h || !out) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (h->filt_ycols <= 0 || (col0 > 0 && h->filt_sm.width <= 0))
        return fail(HC_ERR_ARG, "%s: the last assimilation had no sensor value", who);
    const size_t N = (size_t)h->n_members, width = (size_t)h->filt_ycols;
    std::vector<double> all(N * width);
    if (int rc = filter_hook(h, h->filt_Y, all.data(), all.size(), who)) return rc;
    for (size_t m = 0; m < N; m++) std::copy_n(all.data() + m * width + col0, cols, out + m * cols);
    return HC_OK;
}

int hc_get_filter_loglik(hc_handle *h, double *l) { return filter_sm_hook(h, l, 0, 1, "hc_get_filter_loglik"); }

int hc_get_filter_sm_theta(hc_handle *h, double *theta)
{
    return filter_sm_hook(h, theta, 1, h ? h->filt_sm.width : 0, "hc_get_filter_sm_theta");
}

int hc_set_filter_window(hc_handle *h, int32_t n_offsets, const int32_t *offsets)
{
    if (!h || n_offsets < 0 || (n_offsets > 0 && !offsets)) return fail(HC_ERR_ARG, "hc_set_filter_window: bad argument");
    if (n_offsets > ENKF_SENSORS)
        return fail(HC_ERR_ARG, "hc_set_filter_window: %d offsets, at most %d", (int)n_offsets, ENKF_SENSORS);
    if (n_offsets > 0 && h->enkf_stride > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_window: the EnKF is on (its window: hc_set_enkf_window)");
    if (n_offsets > 0 && h->filt_stride <= 0)
        return fail(HC_ERR_ARG, "hc_set_filter_window: the particle filter is off (hc_set_filter comes first)");
    if (n_offsets > 0 && h->fs_n > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_window: the filter is sharded (hc_set_filter_shard), and the sharded filter "
                                "gathers the water-table indices of the assimilation row only");
    return window_set(h, h->filt_win, h->filt_sm.n, h->filt_stride, fwin_off, ensure_fwin, "hc_set_filter_window", n_offsets,
                      offsets);
}

int hc_get_filter_window_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_filter_window_stats: bad argument");
    return table_copy(h, h->filt_win.table, ensure_fwin, hipMemcpyDeviceToHost, table, n_entries, "hc_get_filter_window_stats");
}

int hc_set_filter_window_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_filter_window_stats: bad argument");
    return table_copy(h, h->filt_win.table, ensure_fwin, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_filter_window_stats");
}

int hc_get_filter_window_capture(hc_handle *h, int32_t *b, int64_t *rows)
{
    if (!h || !b || !rows) return fail(HC_ERR_ARG, "hc_get_filter_window_capture: bad argument");
    return window_capture_get(h, h->filt_win, "hc_get_filter_window_capture", "hc_set_filter_window", b, rows);
}

int hc_set_filter_window_capture(hc_handle *h, const int32_t *b, const int64_t *rows)
{
    if (!h || !b || !rows) return fail(HC_ERR_ARG, "hc_set_filter_window_capture: bad argument");
    if (int rc = window_capture_check(h, h->filt_win, "hc_set_filter_window_capture", "hc_set_filter_window", rows)) return rc;
    for (size_t k = 0; k < (size_t)h->filt_win.n * h->n_members; k++)
        if (b[k] < 0 || b[k] > 65535)
            return fail(HC_ERR_ARG, "hc_set_filter_window_capture: index %d (entry %zu) outside [0, 65535]", (int)b[k], k);
    return window_capture_set(h, h->filt_win, b, rows);
}

int hc_get_filter_window_width(hc_handle *h, int32_t *width, int32_t *slots)
{
    if (!h || !width) return fail(HC_ERR_ARG, "hc_get_filter_window_width: bad argument");
    return window_width(h->filt_win, h->filt_stride > 0 && h->filt_done, width, slots);
}

int hc_set_filter_smoother(hc_handle *h, int32_t stride, int32_t lag)
{
    if (!h) return fail(HC_ERR_ARG, "hc_set_filter_smoother: bad argument");
    if (stride < 0) return fail(HC_ERR_ARG, "hc_set_filter_smoother: stride = %d must be >= 0", (int)stride);
    if (stride > 0 && (lag < 0 || lag > HC_SMOOTHER_MAX_LAG))
        return fail(HC_ERR_ARG, "hc_set_filter_smoother: lag = %d outside [0, %d] record rows", (int)lag, HC_SMOOTHER_MAX_LAG);
    if (stride > 0 && h->enkf_stride > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_smoother: the EnKF is on (the smoother follows the particle filter's ancestry)");
    if (stride > 0 && h->filt_stride <= 0)
        return fail(HC_ERR_ARG, "hc_set_filter_smoother: the particle filter is off (hc_set_filter comes first)");
    if (stride > 0 && h->fs_n > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_smoother: the filter is sharded (hc_set_filter_shard), and the routed columns "
                                "do not carry the smoother's ring");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    smoother_off(h);
    if (stride == 0) return HC_OK;
    h->smo_stride = stride;
    h->smo_lag = lag;
    const int rc = ensure_smoother(h);
    if (rc != HC_OK) smoother_off(h);            // refused: off
    return rc;
}

int hc_get_filter_smoother_layout(hc_handle *h, int32_t *stride, int32_t *lag, int64_t *n_srow)
{
    if (!h || !stride || !lag || !n_srow) return fail(HC_ERR_ARG, "hc_get_filter_smoother_layout: bad argument");
    *stride = h->smo_stride;
    *lag = h->smo_lag;
    *n_srow = h->smo_stride > 0 && h->have_forcing ? smoother_rows(h) : 0;
    return HC_OK;
}

int hc_get_filter_smoother_hist(hc_handle *h, int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_filter_smoother_hist: bad argument");
    return table_copy(h, h->smo_hist, ensure_smoother, hipMemcpyDeviceToHost, table, n_entries, "hc_get_filter_smoother_hist");
}

int hc_set_filter_smoother_hist_table(hc_handle *h, const int32_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_filter_smoother_hist_table: bad argument");
    return table_copy(h, h->smo_hist, ensure_smoother, hipMemcpyHostToDevice, const_cast<int32_t *>(table), n_entries,
                      "hc_set_filter_smoother_hist_table");
}

int hc_get_filter_smoother_paths(hc_handle *h, int64_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_filter_smoother_paths: bad argument");
    return table_copy(h, h->smo_paths, ensure_smoother, hipMemcpyDeviceToHost, table, n_entries,
                      "hc_get_filter_smoother_paths");
}

int hc_set_filter_smoother_paths(hc_handle *h, const int64_t *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_filter_smoother_paths: bad argument");
    return table_copy(h, h->smo_paths, ensure_smoother, hipMemcpyHostToDevice, const_cast<int64_t *>(table), n_entries,
                      "hc_set_filter_smoother_paths");
}

int hc_get_filter_smoother_ring(hc_handle *h, int32_t *w, int64_t *id, int64_t *rows, int64_t *last_row)
{
    if (!h || !w || !id || !rows || !last_row) return fail(HC_ERR_ARG, "hc_get_filter_smoother_ring: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_smoother(h)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->n_members;
    std::vector<unsigned short> hw(N);
    std::vector<unsigned> hid(N);
    for (int k = 0; k <= h->smo_lag; k++) {
        rows[k] = h->smo_row[(size_t)k];
        if (rows[k] >= 0) {
            HIP_TRY(hipMemcpy(hw.data(), h->smo_w.p + (size_t)k * N, N * sizeof(unsigned short), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(hid.data(), h->smo_id.p + (size_t)k * N, N * sizeof(unsigned), hipMemcpyDeviceToHost));
            for (size_t m = 0; m < N; m++) w[(size_t)k * N + m] = (int32_t)hw[m], id[(size_t)k * N + m] = (int64_t)hid[m];
        } else {
            std::fill_n(w + (size_t)k * N, N, (int32_t)0);
            std::fill_n(id + (size_t)k * N, N, (int64_t)0);
        }
    }
    *last_row = h->smo_last;
    return HC_OK;
}

int hc_set_filter_smoother_ring(hc_handle *h, const int32_t *w, const int64_t *id, const int64_t *rows, int64_t last_row)
{
    if (!h || !w || !id || !rows) return fail(HC_ERR_ARG, "hc_set_filter_smoother_ring: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_smoother(h)) return rc;
    const size_t N = (size_t)h->n_members, K1 = (size_t)h->smo_lag + 1;
    const int64_t mpp = h->n_members / h->n_points, s = h->smo_stride;
    if (last_row < -1 || last_row >= h->n_rows)
        return fail(HC_ERR_ARG, "hc_set_filter_smoother_ring: last row %lld outside [-1, %lld)", (long long)last_row,
                    (long long)h->n_rows);
    for (size_t k = 0; k < K1; k++) {
        if (rows[k] == -1) continue;
        if (rows[k] < 1 || rows[k] >= h->n_rows || rows[k] % s != 0 || (size_t)(rows[k] / s) % K1 != k)
            return fail(HC_ERR_ARG, "hc_set_filter_smoother_ring: row %lld is not a record row of plane %zu",
                        (long long)rows[k], k);
        for (size_t m = 0; m < N; m++) {
            if (w[k * N + m] < 0 || w[k * N + m] > 65535)
                return fail(HC_ERR_ARG, "hc_set_filter_smoother_ring: index %d (plane %zu, member %zu) outside [0, 65535]",
                            (int)w[k * N + m], k, m);
            if (id[k * N + m] < 0 || id[k * N + m] >= mpp)
                return fail(HC_ERR_ARG, "hc_set_filter_smoother_ring: id %lld (plane %zu, member %zu) outside [0, %lld)",
                            (long long)id[k * N + m], k, m, (long long)mpp);
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<unsigned short> hw(K1 * N);
    std::vector<unsigned> hid(K1 * N);
    for (size_t e = 0; e < K1 * N; e++) {
        const bool live = rows[e / N] >= 0;
        hw[e] = live ? (unsigned short)w[e] : 0;
        hid[e] = live ? (unsigned)id[e] : 0;
    }
    HIP_TRY(hipMemcpy(h->smo_w.p, hw.data(), hw.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->smo_id.p, hid.data(), hid.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    h->smo_row.assign(rows, rows + K1);
    h->smo_last = last_row;
    return HC_OK;
}

int hc_filter_smoother_flush(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_filter_smoother_flush: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure_smoother(h)) return rc;
    std::vector<int64_t> pending;
    for (const int64_t r : h->smo_row)
        if (r >= 0) pending.push_back(r);
    std::sort(pending.begin(), pending.end());
    for (const int64_t r : pending)
        if (int rc = smoother_emit(h, r / h->smo_stride, std::max(h->smo_last, r))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return HC_OK;
}

int hc_reset_filter_smoother(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "hc_reset_filter_smoother: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->smo_hist.invalidate();
    h->smo_paths.invalidate();
    return ensure_smoother(h);
}

}  // extern "C"
namespace {
// the argument checks the two shard entry points share; n_global through *np
int filter_shard_check(const hc_handle *h, int32_t n_shards, const int64_t *bounds, int32_t index, const char *who, int64_t *np)
{
    if (h->filt_stride <= 0) return fail(HC_ERR_ARG, "%s: the particle filter is off (hc_set_filter comes first)", who);
    if (h->n_points > 1)
        return fail(HC_ERR_ARG, "%s: the handle holds %d points (a shard is a part of one point's members)", who, h->n_points);
    if (n_shards < 1 || !bounds) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (bounds[0] != 0) return fail(HC_ERR_ARG, "%s: bounds[0] = %lld, the bounds must start at 0", who, (long long)bounds[0]);
    for (int32_t s = 0; s < n_shards; s++)
        if (bounds[s + 1] <= bounds[s])
            return fail(HC_ERR_ARG, "%s: bounds[%d] = %lld after %lld, the bounds must be strictly increasing", who, s + 1,
                        (long long)bounds[s + 1], (long long)bounds[s]);
    if (index < 0 || index >= n_shards)
        return fail(HC_ERR_ARG, "%s: index = %d lies outside [0, %d)", who, index, n_shards);
    if (bounds[n_shards] > INT32_MAX)
        return fail(HC_ERR_ARG, "%s: %lld members of the point exceed 2^31 - 1", who, (long long)bounds[n_shards]);
    if (h->n_members != bounds[index + 1] - bounds[index])
        return fail(HC_ERR_ARG, "%s: the handle holds %lld members, shard %d has [%lld, %lld)", who, (long long)h->n_members,
                    index, (long long)bounds[index], (long long)bounds[index + 1]);
    if (h->philox && h->member_offset != bounds[index])
        return fail(HC_ERR_ARG, "%s: shard %d starts at member %lld, but hc_set_noise_philox keys the members from %lld", who,
                    index, (long long)bounds[index], (long long)h->member_offset);
    *np = bounds[n_shards];
    return HC_OK;
}
}  // namespace
extern "C" {

int hc_get_filter_shard_words(hc_handle *h, int32_t n_shards, const int64_t *bounds, int32_t index, int64_t *n_words)
{
    if (!h || !n_words) return fail(HC_ERR_ARG, "hc_get_filter_shard_words: bad argument");
    int64_t np = 0;
    if (int rc = filter_shard_check(h, n_shards, bounds, index, "hc_get_filter_shard_words", &np)) return rc;
    *n_words = filter_shard_layout(np, h->n_members, n_shards, h->p.dim_d).words;
    return HC_OK;
}

int hc_set_filter_shard(hc_handle *h, int32_t n_shards, const int64_t *bounds, int32_t index, void *device_buf,
                        int64_t n_words, hc_enkf_exchange_fn gather, hc_filter_route_fn route, void *ctx)
{
    if (!h || n_shards < 0) return fail(HC_ERR_ARG, "hc_set_filter_shard: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    filter_shard_off(h);
    if (n_shards == 0) return HC_OK;
    int64_t np = 0;
    if (int rc = filter_shard_check(h, n_shards, bounds, index, "hc_set_filter_shard", &np)) return rc;
    if (h->filt_sm.n > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: a soil-moisture record is set (hc_set_filter_soil_moisture), and the "
                                "sharded filter gathers water-table indices only");
    if (h->filt_win.n > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: window offsets are set (hc_set_filter_window), and the sharded filter "
                                "gathers the water-table indices of the assimilation row only");
    if (h->rj_delta > 0.0)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: the base vectors are rejuvenated (hc_set_filter_rejuvenation), and the "
                                "sharded filter gathers water-table indices only: their moments would need an exchange of "
                                "their own");
    if (h->smo_stride > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: the smoother is set (hc_set_filter_smoother), and the routed columns do "
                                "not carry its ring");
    if (h->per_n > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: period totals are set (hc_set_period_totals), and the routed columns do "
                                "not carry the members' accumulators");
    if (h->upt_layers > 0)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: the root uptake is set (hc_set_root_uptake), and the routed columns do "
                                "not carry the members' accumulators");
    if (h->fp_on)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: the forcing is perturbed (hc_set_forcing_perturbation), and the routed "
                                "columns do not carry the members' forcing state");
    if (!device_buf || !gather || !route) return fail(HC_ERR_ARG, "hc_set_filter_shard: NULL buffer or callback");
    const int64_t need = filter_shard_layout(np, h->n_members, n_shards, h->p.dim_d).words;
    if (n_words < need)
        return fail(HC_ERR_ARG, "hc_set_filter_shard: a buffer of %lld words, %lld needed (hc_get_filter_shard_words)",
                    (long long)n_words, (long long)need);
    std::vector<long long> b(bounds, bounds + n_shards + 1);
    if (h->fs_bounds_dev.ensure(b.size())) return HC_ERR_DEVICE;
    HIP_TRY(hipMemcpy(h->fs_bounds_dev.p, b.data(), b.size() * 8, hipMemcpyHostToDevice));
    h->fs_bounds = b;
    h->fs_n = n_shards;
    h->fs_index = index;
    h->fs_buf = static_cast<long long *>(device_buf);
    h->fs_words = n_words;
    h->fs_gather = gather;
    h->fs_route = route;
    h->fs_ctx = ctx;
    return HC_OK;
}

int hc_get_filter_shard(hc_handle *h, int32_t *n_shards, int32_t *index, int64_t *n_global)
{
    if (!h || !n_shards || !index || !n_global) return fail(HC_ERR_ARG, "hc_get_filter_shard: bad argument");
    *n_shards = h->fs_n;
    *index = h->fs_index;
    *n_global = h->fs_n > 0 ? (int64_t)h->fs_bounds[(size_t)h->fs_n] : 0;
    return HC_OK;
}

int hc_set_enkf(hc_handle *h, int32_t stride, double sigma_cm, double localisation_cm, uint64_t seed)
{
    if (!h || stride < 0) return fail(HC_ERR_ARG, "hc_set_enkf: bad argument");
    if (stride > 0 && h->filt_stride > 0)
        return fail(HC_ERR_ARG, "hc_set_enkf: the particle filter is on (hc_set_filter with stride 0 turns it off)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    enkf_off(h);
    if (stride == 0) return HC_OK;
    if (!(std::isfinite(sigma_cm) && sigma_cm > 0.0))
        return fail(HC_ERR_ARG, "hc_set_enkf: sigma_cm = %g must be finite and > 0", sigma_cm);
    if (!(std::isfinite(localisation_cm) && localisation_cm >= 0.0))
        return fail(HC_ERR_ARG, "hc_set_enkf: localisation_cm = %g must be finite and >= 0", localisation_cm);
    StepArgs A;
    if (int rc = fill_args(h, A)) return rc;     // column, forcing, members and noise are in place; point keys uploaded
    if (h->n_rows > (int64_t)UINT32_MAX) return fail(HC_ERR_ARG, "hc_set_enkf: %lld forcing rows exceed 2^32 - 1", (long long)h->n_rows);
    h->enkf_stride = stride;
    h->enkf_sigma = sigma_cm;
    h->enkf_loc = localisation_cm;
    h->enkf_seed = seed;
    const int rc = ensure_enkf(h);
    if (rc != HC_OK) enkf_off(h);                // refused: off
    return rc;
}

int hc_get_enkf_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_enkf_stats: bad argument");
    return table_copy(h, h->enkf, ensure_enkf, hipMemcpyDeviceToHost, table, n_entries, "hc_get_enkf_stats");
}

int hc_set_enkf_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_enkf_stats: bad argument");
    return table_copy(h, h->enkf, ensure_enkf, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_enkf_stats");
}

// What the last analysis was (test hooks): refuses in `who`'s name unless one has run since hc_set_enkf and, as asked,
// the noise field took part in it, it was the square-root one, it relaxed psi
static int enkf_last(const hc_handle *h, const char *who, bool noise = false, bool root = false, bool relaxed = false)
{
    const bool done = h->enkf_stride > 0 && h->enkf_done;
    if (noise && !(done && h->enkf_nz && h->nz_done)) return fail(HC_ERR_ARG, "%s: no analysis since hc_set_enkf_noise_field", who);
    if (root && !(done && h->enkf_last_method == 1)) return fail(HC_ERR_ARG, "%s: no square-root analysis since hc_set_enkf", who);
    if (relaxed && !(done && h->enkf_last_relaxed)) return fail(HC_ERR_ARG, "%s: no relaxed analysis since hc_set_enkf", who);
    if (!done) return fail(HC_ERR_ARG, "%s: no analysis since hc_set_enkf", who);
    return HC_OK;
}

// the last analysis's buffers (test hooks): `rows` rows of `len` doubles, `pitch` apart on the device
static int enkf_hook(hc_handle *h, const double *src, double *out, size_t rows, size_t len, size_t pitch, const char *who)
{
    if (!h || !out) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (int rc = enkf_last(h, who)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (pitch == len) {
        HIP_TRY(hipMemcpy(out, src, rows * len * 8, hipMemcpyDeviceToHost));
        return HC_OK;
    }
    std::vector<double> all((rows - 1) * pitch + len);
    HIP_TRY(hipMemcpy(all.data(), src, all.size() * 8, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; r++) std::copy_n(all.data() + r * pitch, len, out + r * len);
    return HC_OK;
}

// the well's column of the gain [P][m'][D] and of Y [N][m']
int hc_get_enkf_gain(hc_handle *h, double *gain)
{
    const size_t P = h ? (size_t)h->n_points : 0, D = h ? (size_t)h->p.dim_d : 0;
    return enkf_hook(h, h ? h->enkf_psi.gain.p : nullptr, gain, P, D, h ? h->enkf_width * D : 0, "hc_get_enkf_gain");
}

int hc_get_enkf_y(hc_handle *h, double *y)
{
    return enkf_hook(h, h ? h->enkf_Y.p : nullptr, y, h ? (size_t)h->n_members : 0, 1, h ? h->enkf_width : 0,
                     "hc_get_enkf_y");
}

// the square-root analysis draws nothing: its eps do not exist
static int eps_check(hc_handle *h, const char *who)
{
    if (h && h->enkf_stride > 0 && h->enkf_done && h->enkf_last_method == 1)
        return fail(HC_ERR_ARG, "%s: the last analysis was the square-root one, which draws nothing", who);
    return HC_OK;
}

int hc_get_enkf_eps(hc_handle *h, double *eps)
{
    if (int rc = eps_check(h, "hc_get_enkf_eps")) return rc;
    return enkf_hook(h, h ? h->enkf_eps.p : nullptr, eps, 1, h ? (size_t)h->n_members : 0, h ? (size_t)h->n_members : 0,
                     "hc_get_enkf_eps");
}

int hc_set_enkf_soil_moisture(hc_handle *h, int32_t n_sensors, const int32_t *nodes, const double *values,
                              const double *sigma)
{
    if (!h || n_sensors < 0) return fail(HC_ERR_ARG, "hc_set_enkf_soil_moisture: bad argument");
    if (n_sensors > ENKF_SENSORS)
        return fail(HC_ERR_ARG, "hc_set_enkf_soil_moisture: %d sensors, at most %d", (int)n_sensors, ENKF_SENSORS);
    if (n_sensors > 0 && h->filt_stride > 0)
        return fail(HC_ERR_ARG, "hc_set_enkf_soil_moisture: the particle filter is on");
    if (n_sensors > 0 && h->enkf_stride <= 0)
        return fail(HC_ERR_ARG, "hc_set_enkf_soil_moisture: the EnKF is off (hc_set_enkf comes first)");
    return record_set(h, h->enkf_sm, h->enkf_win.n, sm_off, ensure_sm, "hc_set_enkf_soil_moisture", n_sensors, nodes, values,
                      sigma);
}

int hc_get_enkf_sm_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_enkf_sm_stats: bad argument");
    return table_copy(h, h->enkf_sm.table, ensure_sm, hipMemcpyDeviceToHost, table, n_entries, "hc_get_enkf_sm_stats");
}

int hc_set_enkf_sm_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_enkf_sm_stats: bad argument");
    return table_copy(h, h->enkf_sm.table, ensure_sm, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_enkf_sm_stats");
}

int hc_get_enkf_sm_width(hc_handle *h, int32_t *width)
{
    if (!h || !width) return fail(HC_ERR_ARG, "hc_get_enkf_sm_width: bad argument");
    *width = h->enkf_sm.n > 0 ? h->enkf_sm.width : 0;
    return HC_OK;
}

// the last analysis's buffers when it had sensor values (test hooks)
static int sm_check(hc_handle *h, const double *out, const char *who)
{
    if (!h || !out) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (h->enkf_sm.n <= 0 || h->enkf_sm.width <= 0) return fail(HC_ERR_ARG, "%s: the last analysis had no sensor value", who);
    return HC_OK;
}

static int sm_hook(hc_handle *h, const double *src, double *out, size_t count, const char *who)
{
    if (int rc = sm_check(h, out, who)) return rc;
    return enkf_hook(h, src, out, 1, count, count, who);
}

// the well's and the sensors' columns of Y [N][m']
int hc_get_enkf_sm_y(hc_handle *h, double *y)
{
    if (int rc = sm_check(h, y, "hc_get_enkf_sm_y")) return rc;
    return enkf_hook(h, h->enkf_Y.p, y, (size_t)h->n_members, (size_t)h->enkf_sm.width, (size_t)h->enkf_width, "hc_get_enkf_sm_y");
}

// a gain (`dev`: the gain or the reduced gain) is [P][m'][D] on the device, [P][D][.] at the C-ABI: its first `cols` columns
static int gain_hook(hc_handle *h, const double *dev, double *gain, size_t cols, const char *who)
{
    const size_t P = (size_t)h->n_points, D = (size_t)h->p.dim_d, W = (size_t)h->enkf_width;
    std::vector<double> k(P * W * D);
    if (int rc = enkf_hook(h, dev, k.data(), 1, k.size(), k.size(), who)) return rc;
    for (size_t p = 0; p < P; p++)
        for (size_t i = 0; i < cols; i++)
            for (size_t d = 0; d < D; d++) gain[(p * D + d) * cols + i] = k[(p * W + i) * D + d];
    return HC_OK;
}

int hc_get_enkf_sm_gain(hc_handle *h, double *gain)
{
    if (int rc = sm_check(h, gain, "hc_get_enkf_sm_gain")) return rc;
    return gain_hook(h, h->enkf_psi.gain.p, gain, (size_t)h->enkf_sm.width, "hc_get_enkf_sm_gain");
}

int hc_get_enkf_sm_eps(hc_handle *h, double *eps)
{
    if (int rc = eps_check(h, "hc_get_enkf_sm_eps")) return rc;
    return sm_hook(h, h ? h->enkf_eps_s.p : nullptr, eps, h ? (size_t)h->n_members * h->enkf_sm.n : 0, "hc_get_enkf_sm_eps");
}

int hc_set_enkf_window(hc_handle *h, int32_t n_offsets, const int32_t *offsets)
{
    if (!h || n_offsets < 0 || (n_offsets > 0 && !offsets)) return fail(HC_ERR_ARG, "hc_set_enkf_window: bad argument");
    if (n_offsets > ENKF_SENSORS)
        return fail(HC_ERR_ARG, "hc_set_enkf_window: %d offsets, at most %d", (int)n_offsets, ENKF_SENSORS);
    if (n_offsets > 0 && h->enkf_stride <= 0)
        return fail(HC_ERR_ARG, "hc_set_enkf_window: the EnKF is off (hc_set_enkf comes first)");
    return window_set(h, h->enkf_win, h->enkf_sm.n, h->enkf_stride, win_off, ensure_win, "hc_set_enkf_window", n_offsets,
                      offsets);
}

int hc_get_enkf_window_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_enkf_window_stats: bad argument");
    return table_copy(h, h->enkf_win.table, ensure_win, hipMemcpyDeviceToHost, table, n_entries, "hc_get_enkf_window_stats");
}

int hc_set_enkf_window_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_enkf_window_stats: bad argument");
    return table_copy(h, h->enkf_win.table, ensure_win, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_enkf_window_stats");
}

int hc_get_enkf_window_capture(hc_handle *h, double *y, int64_t *rows)
{
    if (!h || !y || !rows) return fail(HC_ERR_ARG, "hc_get_enkf_window_capture: bad argument");
    return window_capture_get(h, h->enkf_win, "hc_get_enkf_window_capture", "hc_set_enkf_window", y, rows);
}

int hc_set_enkf_window_capture(hc_handle *h, const double *y, const int64_t *rows)
{
    if (!h || !y || !rows) return fail(HC_ERR_ARG, "hc_set_enkf_window_capture: bad argument");
    if (int rc = window_capture_check(h, h->enkf_win, "hc_set_enkf_window_capture", "hc_set_enkf_window", rows)) return rc;
    return window_capture_set(h, h->enkf_win, y, rows);
}

int hc_get_enkf_width(hc_handle *h, int32_t *width)
{
    if (!h || !width) return fail(HC_ERR_ARG, "hc_get_enkf_width: bad argument");
    *width = h->enkf_stride > 0 && h->enkf_done ? h->enkf_width : 0;
    return HC_OK;
}

int hc_get_enkf_window_width(hc_handle *h, int32_t *width, int32_t *slots)
{
    if (!h || !width) return fail(HC_ERR_ARG, "hc_get_enkf_window_width: bad argument");
    return window_width(h->enkf_win, h->enkf_stride > 0 && h->enkf_done, width, slots);
}

// the last analysis's buffers when it had lagged columns (test hooks)
static int win_check(hc_handle *h, const double *out, const char *who)
{
    if (!h || !out) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (h->enkf_win.n <= 0 || h->enkf_win.last.empty()) return fail(HC_ERR_ARG, "%s: the last analysis had no lagged row", who);
    return HC_OK;
}

int hc_get_enkf_window_y(hc_handle *h, double *y)
{
    if (int rc = win_check(h, y, "hc_get_enkf_window_y")) return rc;
    const size_t mw = h->enkf_win.last.size(), W = (size_t)h->enkf_width;
    return enkf_hook(h, h->enkf_Y.p + (W - mw), y, (size_t)h->n_members, mw, W, "hc_get_enkf_window_y");
}

int hc_get_enkf_window_eps(hc_handle *h, double *eps)
{
    if (int rc = eps_check(h, "hc_get_enkf_window_eps")) return rc;
    if (int rc = win_check(h, eps, "hc_get_enkf_window_eps")) return rc;
    const size_t n = (size_t)h->n_members * h->enkf_win.last.size();
    return enkf_hook(h, h->enkf_eps_w.p, eps, 1, n, n, "hc_get_enkf_window_eps");
}

int hc_get_enkf_window_gain(hc_handle *h, double *gain)
{
    if (!h || !gain) return fail(HC_ERR_ARG, "hc_get_enkf_window_gain: bad argument");
    return gain_hook(h, h->enkf_psi.gain.p, gain, (size_t)h->enkf_width, "hc_get_enkf_window_gain");
}

int hc_get_enkf_shard_words(hc_handle *h, int64_t n_global, int64_t *n_words)
{
    if (!h || !n_words || n_global < 1) return fail(HC_ERR_ARG, "hc_get_enkf_shard_words: bad argument");
    if (h->enkf_stride <= 0) return fail(HC_ERR_ARG, "hc_get_enkf_shard_words: the EnKF is off (hc_set_enkf)");
    *n_words = shard_words_needed(h, n_global);
    return HC_OK;
}

int hc_set_enkf_shard(hc_handle *h, int64_t n_global, int64_t first_global, void *device_buf, int64_t n_words,
                      hc_enkf_exchange_fn fn, void *ctx)
{
    if (!h || n_global < 0) return fail(HC_ERR_ARG, "hc_set_enkf_shard: bad argument");
    if (n_global == 0) {
        shard_off(h);
        return HC_OK;
    }
    if (h->enkf_stride <= 0) return fail(HC_ERR_ARG, "hc_set_enkf_shard: the EnKF is off (hc_set_enkf comes first)");
    if (h->enkf_nz)
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: the noise field is on (hc_set_enkf_noise_field), and the exchanged "
                                "partials cover psi only");
    if (h->enkf_fg)
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: the forcing analysis is on (hc_set_enkf_forcing), and the exchanged "
                                "partials cover psi only");
    if (h->n_points > 1)
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: the handle holds %d points (a shard is a part of one point's members)",
                    h->n_points);
    const int64_t N = h->n_members;
    if (first_global < 0 || first_global % ENKF_TILE != 0)
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: first_global = %lld must be a multiple of %d", (long long)first_global,
                    ENKF_TILE);
    if (first_global + N > n_global)
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: members [%lld, %lld) lie outside the point's %lld",
                    (long long)first_global, (long long)(first_global + N), (long long)n_global);
    if (first_global + N < n_global && N % ENKF_TILE != 0)
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: %lld members on a shard that is not the point's last must be a "
                    "multiple of %d", (long long)N, ENKF_TILE);
    if (h->philox && h->member_offset != first_global)
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: first_global = %lld, but hc_set_noise_philox keys the members from %lld",
                    (long long)first_global, (long long)h->member_offset);
    if (!device_buf || !fn) return fail(HC_ERR_ARG, "hc_set_enkf_shard: NULL buffer or callback");
    if (n_words < shard_words_needed(h, n_global))
        return fail(HC_ERR_ARG, "hc_set_enkf_shard: a buffer of %lld doubles, %lld needed (hc_get_enkf_shard_words)",
                    (long long)n_words, (long long)shard_words_needed(h, n_global));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->shard_global = n_global;
    h->shard_first = first_global;
    h->shard_buf = static_cast<double *>(device_buf);
    h->shard_words = n_words;
    h->shard_fn = fn;
    h->shard_ctx = ctx;
    return HC_OK;
}

int hc_get_enkf_shard(hc_handle *h, int64_t *n_global, int64_t *first_global)
{
    if (!h || !n_global || !first_global) return fail(HC_ERR_ARG, "hc_get_enkf_shard: bad argument");
    *n_global = h->shard_global;
    *first_global = h->shard_first;
    return HC_OK;
}

int hc_set_enkf_method(hc_handle *h, int32_t method, double relaxation)
{
    if (!h) return fail(HC_ERR_ARG, "hc_set_enkf_method: bad argument");
    if (h->enkf_stride <= 0) return fail(HC_ERR_ARG, "hc_set_enkf_method: the EnKF is off (hc_set_enkf comes first)");
    if (method != 0 && method != 1)
        return fail(HC_ERR_ARG, "hc_set_enkf_method: method = %d must be 0 (stochastic) or 1 (square root)", (int)method);
    if (!(std::isfinite(relaxation) && relaxation >= 0.0 && relaxation <= 1.0))
        return fail(HC_ERR_ARG, "hc_set_enkf_method: relaxation = %g must be finite and in [0, 1]", relaxation);
    h->enkf_method = method;
    h->enkf_alpha = relaxation;
    return HC_OK;
}

int hc_get_enkf_method(hc_handle *h, int32_t *method, double *relaxation)
{
    if (!h || !method || !relaxation) return fail(HC_ERR_ARG, "hc_get_enkf_method: bad argument");
    *method = h->enkf_stride > 0 ? h->enkf_method : 0;
    *relaxation = h->enkf_stride > 0 ? h->enkf_alpha : 0.0;
    return HC_OK;
}

// the reduced gain is [P][m'][D] on the device, [P][D][m'] at the C-ABI (as hc_get_enkf_sm_gain)
int hc_get_enkf_sqrt_gain(hc_handle *h, double *gain)
{
    if (!h || !gain) return fail(HC_ERR_ARG, "hc_get_enkf_sqrt_gain: bad argument");
    if (int rc = enkf_last(h, "hc_get_enkf_sqrt_gain", false, true)) return rc;
    return gain_hook(h, h->enkf_psi.rgain.p, gain, (size_t)h->enkf_width, "hc_get_enkf_sqrt_gain");
}

// an array of the last analysis as on the device, psi's or (noise) z's: a gain [P][m'][D] or (shift) the shift [P][D]
static int vec_hook(hc_handle *h, bool noise, DevBuf<double> EnkfVec::*src, double *out, bool root, bool shift, const char *who)
{
    if (!h || !out) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (int rc = enkf_last(h, who, noise, root)) return rc;
    const size_t n = (size_t)h->n_points * h->p.dim_d * (shift ? 1 : (size_t)h->enkf_width);
    return enkf_hook(h, ((noise ? h->enkf_z : h->enkf_psi).*src).p, out, 1, n, n, who);
}

int hc_get_enkf_sqrt_shift(hc_handle *h, double *shift)
{
    return vec_hook(h, false, &EnkfVec::dbar, shift, true, true, "hc_get_enkf_sqrt_shift");
}

int hc_get_enkf_relaxation(hc_handle *h, double *sigma_b, double *sigma_a, double *factor)
{
    if (!h || !sigma_b || !sigma_a || !factor) return fail(HC_ERR_ARG, "hc_get_enkf_relaxation: bad argument");
    if (int rc = enkf_last(h, "hc_get_enkf_relaxation", false, false, true)) return rc;
    const size_t n = (size_t)h->n_points * h->p.dim_d;
    double *out[3] = {sigma_b, sigma_a, factor};
    for (int k = 0; k < 3; k++)
        if (int rc = enkf_hook(h, h->enkf_psi.relax.p + k * n, out[k], 1, n, n, "hc_get_enkf_relaxation")) return rc;
    return HC_OK;
}

// ---- the noise field in the analysis (include/hydrocol.h)
int hc_set_enkf_noise_field(hc_handle *h, int32_t on, double relaxation)
{
    if (!h || (on != 0 && on != 1)) return fail(HC_ERR_ARG, "hc_set_enkf_noise_field: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!on) {
        nz_off(h);
        return HC_OK;
    }
    if (h->enkf_stride <= 0) return fail(HC_ERR_ARG, "hc_set_enkf_noise_field: the EnKF is off (hc_set_enkf comes first)");
    if (h->shard_global > 0)
        return fail(HC_ERR_ARG, "hc_set_enkf_noise_field: the analysis is sharded (hc_set_enkf_shard), and the exchanged "
                                "partials cover psi only");
    if (!(std::isfinite(relaxation) && relaxation >= 0.0 && relaxation <= 1.0))
        return fail(HC_ERR_ARG, "hc_set_enkf_noise_field: relaxation = %g must be finite and in [0, 1]", relaxation);
    StepArgs A;
    if (int rc = fill_args(h, A)) return rc;     // column, forcing, members and noise are in place; point keys uploaded
    const bool was_on = h->enkf_nz;
    h->enkf_nz = true;
    h->enkf_nz_alpha = relaxation;
    int rc = ensure_nz(h);
    if (rc == HC_OK && h->philox && !was_on && !h->ncorr) {
        // as hc_set_filter: the base vectors the kernel's Philox path would build, from here on carried like the caller's
        const size_t total = (size_t)h->n_members * h->p.dim_d;
        rc = h->base.ensure(total);
        if (rc == HC_OK) rc = launch_noise_fill(h, h->base.p, 1, nullptr, h->nscale.p);
        if (rc == HC_OK) {
            const hipError_t e = hipGetLastError();
            const hipError_t e2 = hipStreamSynchronize(h->stream);
            if (e != hipSuccess || e2 != hipSuccess)
                rc = fail(HC_ERR_DEVICE, "hc_set_enkf_noise_field: base vectors: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        }
    }
    if (rc != HC_OK) nz_off(h);                  // refused: off
    return rc;
}

int hc_get_enkf_noise_field(hc_handle *h, int32_t *on, double *relaxation)
{
    if (!h || !on || !relaxation) return fail(HC_ERR_ARG, "hc_get_enkf_noise_field: bad argument");
    *on = h->enkf_nz ? 1 : 0;
    *relaxation = h->enkf_nz ? h->enkf_nz_alpha : 0.0;
    return HC_OK;
}

int hc_get_enkf_noise_stats(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_enkf_noise_stats: bad argument");
    return table_copy(h, h->enkf_nzt, ensure_nz, hipMemcpyDeviceToHost, table, n_entries, "hc_get_enkf_noise_stats");
}

int hc_set_enkf_noise_stats(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_enkf_noise_stats: bad argument");
    return table_copy(h, h->enkf_nzt, ensure_nz, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_enkf_noise_stats");
}

// the last analysis's gain for the vectors as on the device, the square-root run's reduced gain and its shift
int hc_get_enkf_noise_gain(hc_handle *h, double *gain)
{
    return vec_hook(h, true, &EnkfVec::gain, gain, false, false, "hc_get_enkf_noise_gain");
}

int hc_get_enkf_noise_sqrt_gain(hc_handle *h, double *gain)
{
    return vec_hook(h, true, &EnkfVec::rgain, gain, true, false, "hc_get_enkf_noise_sqrt_gain");
}

int hc_get_enkf_noise_sqrt_shift(hc_handle *h, double *shift)
{
    return vec_hook(h, true, &EnkfVec::dbar, shift, true, true, "hc_get_enkf_noise_sqrt_shift");
}

// ---- the members' forcing state in the analysis (include/hydrocol.h)
int hc_set_enkf_forcing(hc_handle *h, int32_t on, double relaxation)
{
    if (!h || (on != 0 && on != 1)) return fail(HC_ERR_ARG, "hc_set_enkf_forcing: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!on) {
        fg_off(h);
        return HC_OK;
    }
    if (h->enkf_stride <= 0) return fail(HC_ERR_ARG, "hc_set_enkf_forcing: the EnKF is off (hc_set_enkf comes first)");
    if (!h->fp_on)
        return fail(HC_ERR_ARG, "hc_set_enkf_forcing: the forcing is not perturbed (hc_set_forcing_perturbation comes first)");
    if (h->shard_global > 0)
        return fail(HC_ERR_ARG, "hc_set_enkf_forcing: the analysis is sharded (hc_set_enkf_shard), and the exchanged "
                                "partials cover psi only");
    if (!(std::isfinite(relaxation) && relaxation >= 0.0 && relaxation <= 1.0))
        return fail(HC_ERR_ARG, "hc_set_enkf_forcing: relaxation = %g must be finite and in [0, 1]", relaxation);
    h->enkf_fg = true;
    h->enkf_fg_alpha = relaxation;
    const int rc = ensure_fg(h);
    if (rc != HC_OK) fg_off(h);                  // refused: off
    return rc;
}

int hc_get_enkf_forcing(hc_handle *h, int32_t *on, double *relaxation)
{
    if (!h || !on || !relaxation) return fail(HC_ERR_ARG, "hc_get_enkf_forcing: bad argument");
    *on = h->enkf_fg ? 1 : 0;
    *relaxation = h->enkf_fg ? h->enkf_fg_alpha : 0.0;
    return HC_OK;
}

int hc_get_enkf_g_table(hc_handle *h, double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_get_enkf_g_table: bad argument");
    return table_copy(h, h->enkf_fgt, ensure_fg, hipMemcpyDeviceToHost, table, n_entries, "hc_get_enkf_g_table");
}

int hc_set_enkf_g_table(hc_handle *h, const double *table, int64_t n_entries)
{
    if (!h || !table) return fail(HC_ERR_ARG, "hc_set_enkf_g_table: bad argument");
    return table_copy(h, h->enkf_fgt, ensure_fg, hipMemcpyHostToDevice, const_cast<double *>(table), n_entries,
                      "hc_set_enkf_g_table");
}

// the last analysis's gain for g as on the device [P][m'][2], the square-root run's reduced gain and its shift [P][2]
static int forcing_hook(hc_handle *h, DevBuf<double> EnkfVec::*src, double *out, bool root, bool shift, const char *who)
{
    if (!h || !out) return fail(HC_ERR_ARG, "%s: bad argument", who);
    if (!(h->enkf_stride > 0 && h->enkf_done && h->enkf_fg && h->fg_done))
        return fail(HC_ERR_ARG, "%s: no analysis since hc_set_enkf_forcing", who);
    if (int rc = enkf_last(h, who, false, root)) return rc;
    const size_t n = (size_t)h->n_points * 2 * (shift ? 1 : (size_t)h->enkf_width);
    return enkf_hook(h, (h->enkf_gv.*src).p, out, 1, n, n, who);
}

int hc_get_enkf_g_gain(hc_handle *h, double *gain)
{
    return forcing_hook(h, &EnkfVec::gain, gain, false, false, "hc_get_enkf_g_gain");
}

int hc_get_enkf_g_sqrt_gain(hc_handle *h, double *gain)
{
    return forcing_hook(h, &EnkfVec::rgain, gain, true, false, "hc_get_enkf_g_sqrt_gain");
}

int hc_get_enkf_g_sqrt_shift(hc_handle *h, double *shift)
{
    return forcing_hook(h, &EnkfVec::dbar, shift, true, true, "hc_get_enkf_g_sqrt_shift");
}

int hc_get_enkf_noise_base(hc_handle *h, double *base, int64_t first, int64_t count)
{
    if (!h || !base || first < 0 || count < 0 || first + count > h->n_members || !(h->enkf_nz && h->philox))
        return fail(HC_ERR_ARG, "hc_get_enkf_noise_base: bad argument (a Philox run with the EnKF's noise field on)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int D = h->p.dim_d;
    HIP_TRY(hipMemcpy(base, h->base.p + (size_t)first * D, (size_t)count * D * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_enkf_noise_base(hc_handle *h, const double *base)
{
    if (!h || !base || !(h->enkf_nz && h->philox))
        return fail(HC_ERR_ARG, "hc_set_enkf_noise_base: bad argument (a Philox run with the EnKF's noise field on)");
    const size_t n = (size_t)h->n_members * h->p.dim_d;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->base.p, base, n * 8, hipMemcpyHostToDevice));
    return HC_OK;
}

// The path's one collective without torch: a single process that drives several devices (one handle each) sums the
// handles' moment tables over RCCL.  RCCL is bound at run time (dlopen), so the library loads on boxes without it and
// a process that already carries an RCCL (torch's) keeps using that one.
namespace {
struct Rccl {
    void *so = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
int load_rccl(Rccl &r)
{
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        r.so = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (r.so) break;
    }
    if (!r.so) return fail(HC_ERR_UNSUPPORTED, "RCCL is not loadable (%s)", dlerror());
    r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(dlsym(r.so, "ncclCommInitAll"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.so, "ncclCommDestroy"));
    r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.so, "ncclGroupStart"));
    r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.so, "ncclGroupEnd"));
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.so, "ncclAllReduce"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.so, "ncclGetErrorString"));
    if (!r.CommInitAll || !r.CommDestroy || !r.GroupStart || !r.GroupEnd || !r.AllReduce || !r.GetErrorString)
        return fail(HC_ERR_UNSUPPORTED, "the RCCL library lacks an entry point this call needs");
    return HC_OK;
}
}  // namespace

int hc_allreduce_moments(hc_handle **handles, int n)
{
    if (!handles || n < 1 || n > 64) return fail(HC_ERR_ARG, "hc_allreduce_moments: bad argument");
    size_t count = 0;
    std::vector<int> devs((size_t)n);
    for (int k = 0; k < n; k++) {
        hc_handle *h = handles[k];
        if (!h) return fail(HC_ERR_ARG, "handle %d is NULL", k);
        HIP_TRY(hipSetDevice(h->device));
        if (int rc = ensure_moments(h)) return rc;
        const size_t c = (size_t)h->moments.n;
        if (k == 0) count = c;
        if (c != count) return fail(HC_ERR_ARG, "handle %d holds a moment table of another shape", k);
        for (int j = 0; j < k; j++)
            if (handles[j]->device == h->device) return fail(HC_ERR_ARG, "handles %d and %d share device %d: one handle per device", j, k, h->device);
        devs[(size_t)k] = h->device;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    Rccl r;
    if (int rc = load_rccl(r)) return rc;
    constexpr int NCCL_INT64 = 4, NCCL_SUM = 0;     // rccl.h: ncclInt64, ncclSum
    std::vector<void *> comms((size_t)n, nullptr);
    int e = r.CommInitAll(comms.data(), n, devs.data());
    if (e != 0) return fail(HC_ERR_DEVICE, "ncclCommInitAll failed: %s", r.GetErrorString(e));
    int bad = 0;
    bad = bad ? bad : r.GroupStart();
    for (int k = 0; k < n && !bad; k++) {
        (void)hipSetDevice(handles[k]->device);
        bad = r.AllReduce(handles[k]->moments.buf.p, handles[k]->moments.buf.p, count, NCCL_INT64, NCCL_SUM, comms[(size_t)k],
                          handles[k]->stream);
    }
    const int ge = r.GroupEnd();
    bad = bad ? bad : ge;
    hipError_t he = hipSuccess;
    for (int k = 0; k < n; k++) {
        (void)hipSetDevice(handles[k]->device);
        const hipError_t e1 = hipStreamSynchronize(handles[k]->stream);
        he = he == hipSuccess ? e1 : he;
    }
    for (int k = 0; k < n; k++) (void)r.CommDestroy(comms[(size_t)k]);
    if (bad) return fail(HC_ERR_DEVICE, "RCCL all-reduce of the moment tables failed: %s", r.GetErrorString(bad));
    HIP_TRY(he);
    return HC_OK;
}

int hc_get_noise_scale(hc_handle *h, double *scale, int64_t first, int64_t count)
{
    if (!h || !scale || first < 0 || count < 0 || first + count > h->n_members || !h->nscale.p)
        return fail(HC_ERR_ARG, "hc_get_noise_scale: bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(scale, h->nscale.p + first, (size_t)count * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_noise_scale(hc_handle *h, const double *scale, int64_t first, int64_t count)
{
    if (!h || !scale || first < 0 || count < 0 || first + count > h->n_members || !h->nscale.p)
        return fail(HC_ERR_ARG, "hc_set_noise_scale: bad argument");
    if (!h->philox) return fail(HC_ERR_ARG, "hc_set_noise_scale: call hc_set_noise_philox first (it resets the scales to 1)");
    if (h->filt_host())
        return fail(HC_ERR_ARG, "hc_set_noise_scale: the particle filter is on and the base vectors carry the damping "
                                "(set the scales before hc_set_filter, or the vectors with hc_set_filter_base)");
    if (h->corr_host())
        return fail(HC_ERR_ARG, "hc_set_noise_scale: a noise correlation is set and the base vectors carry the damping "
                                "(set the scales, like the spin-up, before the correlation: set the correlation after the "
                                "spin-up; or the vectors with hc_set_noise_field_base)");
    if (h->noise_host())
        return fail(HC_ERR_ARG, "hc_set_noise_scale: the EnKF's noise field is on and the base vectors carry the damping "
                                "(set the scales before hc_set_enkf_noise_field, or the vectors with hc_set_enkf_noise_base)");
    for (int64_t k = 0; k < count; k++)
        if (!(scale[k] > 0.0) || !(scale[k] <= 1.0))
            return fail(HC_ERR_ARG, "noise scale %lld = %g is not a product of 0.8 factors in (0, 1]", (long long)(first + k), scale[k]);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->nscale.p + first, scale, (size_t)count * 8, hipMemcpyHostToDevice));
    return HC_OK;
}

int hc_set_point_member_bases(hc_handle *h, const int64_t *base)
{
    if (!h) return fail(HC_ERR_ARG, "NULL handle");
    if (!h->have_column) return fail(HC_ERR_ARG, "hc_set_column must come first");
    if (h->filt_stride > 0 || h->enkf_stride > 0 || h->ncorr) {   // the points' stream keys change: the filters are off
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        assimilation_off(h);
    }
    if (h->fp_on) {              // ... and so is the perturbed forcing, keyed by them
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        forcing_pert_off(h);
    }
    h->base_host.clear();
    if (base) {
        for (int k = 0; k < h->n_points; k++)
            if (base[k] < 0) return fail(HC_ERR_ARG, "member base of point %d is negative", k);
        h->base_host.assign(base, base + h->n_points);
    }
    return HC_OK;
}

// ---- perturbed forcing (include/hydrocol.h)
int hc_set_forcing_perturbation(hc_handle *h, double sigma_precip, double sigma_demand, double phi, double c, uint64_t seed)
{
    if (!h) return fail(HC_ERR_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    forcing_pert_off(h);                          // (and off it stays when the parameters are refused)
    if (!h->have_column || !h->have_forcing || h->n_members <= 0 || !h->psi.p)
        return fail(HC_ERR_ARG, "hc_set_forcing_perturbation: hc_set_column, hc_set_forcing, hc_set_members and hc_set_state "
                                "must come first");
    if (!std::isfinite(sigma_precip) || !std::isfinite(sigma_demand) || !std::isfinite(phi) || !std::isfinite(c))
        return fail(HC_ERR_ARG, "hc_set_forcing_perturbation: sigma = %g, %g, phi = %g, c = %g not finite", sigma_precip,
                    sigma_demand, phi, c);
    if (!(sigma_precip >= 0.0 && sigma_precip <= 1.0) || !(sigma_demand >= 0.0 && sigma_demand <= 1.0))
        return fail(HC_ERR_ARG, "hc_set_forcing_perturbation: sigma = %g, %g outside [0, 1]", sigma_precip, sigma_demand);
    if (!(phi >= 0.0 && phi < 1.0) || !(c > 0.0))
        return fail(HC_ERR_ARG, "hc_set_forcing_perturbation: phi = %g outside [0, 1) or c = %g <= 0", phi, c);
    if (std::fabs(phi * phi + c * c - 1.0) > 1e-12)
        return fail(HC_ERR_ARG, "hc_set_forcing_perturbation: phi = %g, c = %g is no unit-variance step (phi^2 + c^2 = 1)", phi, c);
    if (h->fs_n > 0)
        return fail(HC_ERR_ARG, "hc_set_forcing_perturbation: the particle filter is sharded (hc_set_filter_shard), and the "
                                "routed columns do not carry the members' forcing state");
    if (h->n_members % h->n_points != 0)
        return fail(HC_ERR_ARG, "%lld members do not divide into %d parameter points", (long long)h->n_members, h->n_points);
    h->fp_sigma[0] = sigma_precip;
    h->fp_sigma[1] = sigma_demand;
    h->fp_phi = phi;
    h->fp_c = c;
    h->fp_seed = seed;
    h->fp_on = true;
    return HC_OK;
}

int hc_set_forcing_member_offset(hc_handle *h, int64_t member_offset)
{
    if (!h || member_offset < 0) return fail(HC_ERR_ARG, "hc_set_forcing_member_offset: bad argument");
    if (!h->fp_on)
        return fail(HC_ERR_ARG, "hc_set_forcing_member_offset: the forcing is not perturbed (hc_set_forcing_perturbation)");
    if (h->n_points > 1)
        return fail(HC_ERR_ARG, "hc_set_forcing_member_offset: %d parameter points: their members' ids are those of "
                                "hc_set_point_member_bases", h->n_points);
    if (h->fp_day >= 0)
        return fail(HC_ERR_ARG, "hc_set_forcing_member_offset: rows have been stepped (the state stands at day %lld): set the "
                                "offset first", (long long)h->fp_day);
    h->fp_offset = member_offset;
    return HC_OK;
}

int hc_clear_forcing_perturbation(hc_handle *h)
{
    if (!h) return fail(HC_ERR_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    forcing_pert_off(h);
    return HC_OK;
}

int hc_get_forcing_perturbation(hc_handle *h, int32_t *on, double *sigma_precip, double *sigma_demand, double *phi, double *c,
                                uint64_t *seed)
{
    if (!h || !on) return fail(HC_ERR_ARG, "hc_get_forcing_perturbation: bad argument");
    *on = h->fp_on ? 1 : 0;
    if (!h->fp_on) return HC_OK;
    if (sigma_precip) *sigma_precip = h->fp_sigma[0];
    if (sigma_demand) *sigma_demand = h->fp_sigma[1];
    if (phi) *phi = h->fp_phi;
    if (c) *c = h->fp_c;
    if (seed) *seed = h->fp_seed;
    return HC_OK;
}

int hc_get_forcing_state(hc_handle *h, double *g, int64_t *day)
{
    if (!h || !g || !day) return fail(HC_ERR_ARG, "hc_get_forcing_state: bad argument");
    if (!h->fp_on) return fail(HC_ERR_ARG, "hc_get_forcing_state: the forcing is not perturbed (hc_set_forcing_perturbation)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *day = h->fp_day;
    const size_t n = (size_t)(2 * h->n_members);
    if (h->fp_day < 0) std::fill(g, g + n, 0.0);
    else HIP_TRY(hipMemcpy(g, h->fp_g.p, n * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_set_forcing_state(hc_handle *h, const double *g, int64_t day)
{
    if (!h || !g || day < -1 || day > (int64_t)UINT32_MAX) return fail(HC_ERR_ARG, "hc_set_forcing_state: bad argument");
    if (!h->fp_on) return fail(HC_ERR_ARG, "hc_set_forcing_state: the forcing is not perturbed (hc_set_forcing_perturbation)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t n = (size_t)(2 * h->n_members);
    if (day >= 0) {
        for (size_t i = 0; i < n; i++)
            if (!std::isfinite(g[i])) return fail(HC_ERR_ARG, "hc_set_forcing_state: entry %zu is not finite", i);
        if (h->fp_g.ensure(n)) return HC_ERR_DEVICE;
        HIP_TRY(hipMemcpy(h->fp_g.p, g, n * 8, hipMemcpyHostToDevice));
    }
    h->fp_day = day;
    return HC_OK;
}

int hc_forcing_normals(hc_handle *h, int64_t member, int64_t first_day, int64_t n_days, double *out)
{
    if (!h || !out || member < 0 || first_day < 0 || n_days < 1 || first_day + n_days - 1 > (int64_t)UINT32_MAX)
        return fail(HC_ERR_ARG, "hc_forcing_normals: bad argument");
    if (!h->fp_on) return fail(HC_ERR_ARG, "hc_forcing_normals: the forcing is not perturbed (hc_set_forcing_perturbation)");
    HIP_TRY(hipSetDevice(h->device));
    const size_t n = (size_t)(2 * n_days);
    if (h->scratch_d.ensure(n)) return HC_ERR_DEVICE;
    hipLaunchKernelGGL(forcing_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->scratch_d.p,
                       (unsigned long long)member, (long long)first_day, (long long)n_days, forcing_pert_of(h));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->scratch_d.p, n * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_forcing_factors(hc_handle *h, int64_t first_member, int64_t count, int64_t first_day, int64_t n_days, double *out)
{
    if (!h || !out || first_member < 0 || count < 1 || first_day < 0 || n_days < 1 ||
        first_day + n_days - 1 > (int64_t)UINT32_MAX)
        return fail(HC_ERR_ARG, "hc_forcing_factors: bad argument");
    if (!h->fp_on) return fail(HC_ERR_ARG, "hc_forcing_factors: the forcing is not perturbed (hc_set_forcing_perturbation)");
    if (first_member + count > h->n_members) return fail(HC_ERR_ARG, "hc_forcing_factors: bad member range");
    HIP_TRY(hipSetDevice(h->device));
    const int NP = h->n_points;
    const long long mpp = h->n_members / NP;
    if (NP > 1) {                                 // the points' keys as fill_args uploads them
        if (h->point_base.ensure((size_t)NP)) return HC_ERR_DEVICE;
        std::vector<long long> base(h->base_host);
        if ((int)base.size() != NP) {
            base.resize((size_t)NP);
            for (int k = 0; k < NP; k++) base[(size_t)k] = h->member_offset + (long long)k * mpp;
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(h->point_base.p, base.data(), (size_t)NP * 8, hipMemcpyHostToDevice));
    }
    const size_t n = (size_t)(n_days * 2 * count);
    if (h->scratch_d.ensure(n)) return HC_ERR_DEVICE;
    hipLaunchKernelGGL(forcing_factor_fill_kernel, dim3((unsigned)((2 * count + 255) / 256)), dim3(256), 0, h->stream,
                       (const double *)nullptr, (double *)nullptr, -1LL, 0LL, h->scratch_d.p, (long long)first_member,
                       (long long)count, (long long)first_day, (long long)(first_day + n_days - 1), mpp,
                       NP > 1 ? h->point_base.p : nullptr, forcing_member_offset(h), forcing_pert_of(h));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->scratch_d.p, n * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_get_point_costs(hc_handle *h, uint64_t *cost)
{
    if (!h || !cost) return fail(HC_ERR_ARG, "hc_get_point_costs: bad argument");
    if (!h->have_column) return fail(HC_ERR_ARG, "hc_set_column must come first");
    for (int k = 0; k < h->n_points; k++)
        cost[k] = (size_t)k < h->cost_total.size() ? h->cost_total[(size_t)k] : 0ull;
    return HC_OK;
}

int hc_set_generic_exponents(hc_handle *h, int32_t on)
{
    if (!h) return fail(HC_ERR_ARG, "NULL handle");
    h->force_generic = on != 0;
    return HC_OK;
}

int hc_set_rows_per_launch(hc_handle *h, int32_t rows)
{
    if (!h || rows < 0) return fail(HC_ERR_ARG, "hc_set_rows_per_launch: bad argument");
    h->rows_per_launch = rows;
    return HC_OK;
}

int hc_set_iteration_budget(hc_handle *h, int32_t phase_steps)
{
    if (!h || phase_steps < 1) return fail(HC_ERR_ARG, "hc_set_iteration_budget: bad argument");
    h->max_phase_iterations = phase_steps;
    return HC_OK;
}

int hc_set_scipy_152(hc_handle *h, int32_t on)
{
    if (!h) return fail(HC_ERR_ARG, "hc_set_scipy_152: NULL handle");
    h->scipy_152 = on ? 1 : 0;
    return HC_OK;
}

int hc_rhs(hc_handle *h, int64_t row, int32_t spinup, double *dydt, double *aux)
{
    return hc_rhs_ex(h, row, spinup, HC_RHS_HOOK, dydt, aux, nullptr);
}

int hc_rhs_ex(hc_handle *h, int64_t row, int32_t spinup, int32_t variant, double *dydt, double *aux, double *diag)
{
    if (!h || !dydt) return fail(HC_ERR_ARG, "hc_rhs: NULL argument");
    if (variant != HC_RHS_HOOK && variant != HC_RHS_AS_STEPPED && variant != HC_RHS_HOOK_LAYOUT)
        return fail(HC_ERR_ARG, "hc_rhs_ex: variant %d (0 = hook, 1 = as stepped, 2 = hook on the step kernel's layout)", (int)variant);
    StepArgs A;
    int rc = fill_args(h, A);
    if (rc) return rc;
    if (row < 0 || row >= h->n_rows) return fail(HC_ERR_ARG, "row out of range");
    if (h->n_points != 1) return fail(HC_ERR_UNSUPPORTED, "hc_rhs (test hook) serves one parameter point");
    HIP_TRY(hipSetDevice(h->device));
    const int D = h->p.dim_d;
    const size_t n = (size_t)h->n_members * D, na = (size_t)h->n_members * (3 * (D - 1) + 1);
    const size_t nd = (size_t)h->n_members * 2;
    if (h->scratch_d.ensure(n + na + nd)) return HC_ERR_DEVICE;
    double *const aux_d = h->scratch_d.p + n, *const diag_d = aux_d + na;
    A.spinup = spinup;
    rc = push_io(h);
    if (rc) return rc;
#ifdef HC_PROFILE
    if (const char *e = getenv("HYDROCOL_RHS_REPEAT")) A.n_rows = atoll(e);
#endif
    rc = launch_rhs(h, A, row, variant, h->scratch_d.p, aux ? aux_d : nullptr, diag ? diag_d : nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(dydt, h->scratch_d.p, n * 8, hipMemcpyDeviceToHost));
    if (aux) HIP_TRY(hipMemcpy(aux, aux_d, na * 8, hipMemcpyDeviceToHost));
    if (diag) HIP_TRY(hipMemcpy(diag, diag_d, nd * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_model_nodes(hc_handle *h, double *out, double *qinf)
{
    if (!h || !out) return fail(HC_ERR_ARG, "hc_model_nodes: NULL argument");
    StepArgs A;
    int rc = fill_args(h, A);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const int D = h->p.dim_d;
    const size_t n = (size_t)h->n_members * D;
    if (h->scratch_d.ensure(4 * n + (size_t)h->n_members)) return HC_ERR_DEVICE;
    rc = push_io(h);
    if (rc) return rc;
    hipLaunchKernelGGL(model_nodes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, A,
                       h->node_tabs.p, (int)h->use_special(), h->scratch_d.p, h->scratch_d.p + 4 * n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->scratch_d.p, 4 * n * 8, hipMemcpyDeviceToHost));
    if (qinf) HIP_TRY(hipMemcpy(qinf, h->scratch_d.p + 4 * n, (size_t)h->n_members * 8, hipMemcpyDeviceToHost));
    return HC_OK;
}

int hc_plugin_eval(int device_ordinal, const hc_column_params *p, int64_t n_cells, int64_t n_cols,
                   const double *psi, const double *por, const double *meank, const double *noisec,
                   const double *n_rnd, double *out, double *qinf)
{
    if (!p || !psi || !por || !meank || !noisec || !n_rnd || !out || !qinf || n_cells < 1 || n_cols < 1)
        return fail(HC_ERR_ARG, "hc_plugin_eval: bad argument");
    if (!(p->n > 1.0) || !(p->alpha > 0.0) || !(p->dz > 0.0)) return fail(HC_ERR_ARG, "bad dz / n / alpha");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(HC_ERR_NO_DEVICE, "no HIP device visible (%s): the plugin call has no CPU path",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= count) return fail(HC_ERR_ARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device_ordinal));
    ColumnDev P{};
    P.model = p->model;
    P.theta_res = p->theta_res; P.alpha = p->alpha; P.n = p->n; P.m = p->m; P.psi_sat = p->psi_sat;
    P.epsilon = p->epsilon; P.lambda = p->lambda_exp; P.sigma = p->sigma_noise; P.sat_soil = p->sat_soil;
    P.dz = p->dz; P.inv_dz = 1.0 / p->dz;
    P.mn_alpha = (p->m * p->n) * p->alpha;
    P.inv_m = 1.0 / p->m;
    const int special = (p->model == HC_MODEL_VRETTAS_FUNG && p->n == 2.0 && p->m == 0.5 && p->lambda_exp == 1.0);
    const size_t nk = (size_t)n_cells, tot = nk * (size_t)n_cols;
    DevBuf<double> in, res;
    if (in.ensure(tot + 4 * nk) || res.ensure(4 * tot + (size_t)n_cols)) {
        in.release(); res.release();
        return HC_ERR_DEVICE;
    }
    int rc = [&]() -> int {
        HIP_TRY(hipMemcpy(in.p, psi, tot * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(in.p + tot, por, nk * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(in.p + tot + nk, meank, nk * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(in.p + tot + 2 * nk, noisec, nk * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(in.p + tot + 3 * nk, n_rnd, nk * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(plugin_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, P, special,
                           (long long)n_cells, (long long)n_cols, in.p, in.p + tot, in.p + tot + nk,
                           in.p + tot + 2 * nk, in.p + tot + 3 * nk, res.p, res.p + 4 * tot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, res.p, 4 * tot * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(qinf, res.p + 4 * tot, (size_t)n_cols * 8, hipMemcpyDeviceToHost));
        return HC_OK;
    }();
    in.release();
    res.release();
    return rc;
}

}  // extern "C"
