// mf_job.h -- making and taking apart a training job (ure_job_create / ure_job_destroy).  Host code only; included by mf_train.hip
// after the launch functions, whose headers define the limits checked here (kTouch*, kAhead*, kIdx*).
//
// ure_job_create, in order: check the shards (no HIP call before every refusal has had its say), plan the launches, upload the
// descriptors, make the library-owned memory of touch mode (block_cache.cpp), upload the derived constants.  A refusal comes before
// there is a job; from then on a unique_ptr holds it, so a HIP error at any step takes it apart through ure_job_destroy.
#pragma once
#include <memory>

namespace ure {

// ---- the refusals: pure host functions of the descriptors; 0, or what fail() returned

static int check_descriptor(const ure_shard_t *shards, int k)
{
    const ure_shard_t &S = shards[k];
    const int n_rows = S.n_user + S.n_item;
    const bool ok = S.N > 0 && S.n_user > 0 && S.n_item > 0 && S.batch > 0 && S.epochs > 0 && pow2(S.d) && S.d >= 4 &&
                    S.d <= 256 && S.n_active >= 0 && S.n_active <= n_rows && S.units && S.n_units >= 0 &&
                    S.n_units % (kBlock / lanes_per_row(S.d)) == 0 && S.n_slots >= S.N && S.ent_oid && S.ent_r && S.ent_tag && S.ent_src &&
                    S.file_tag && S.sched && S.U[0] && S.U[1] && S.V[0] && S.V[1] && S.mU && S.mV && (S.perm || S.file_tags) && S.lr && S.sse &&
                    (!S.lazy_rows || (S.U0 && S.V0 && S.lr_host));
    if (!ok) return fail(-1, "ure_job_create: shard %d has an invalid descriptor", k);
    if (S.d != shards[0].d) return fail(-1, "ure_job_create: all shards of a job share d");
    const int steps = make_shard_aux(S).steps;
    if (steps > 65534) return fail(-1, "ure_job_create: shard %d needs %lld steps/epoch (> 65534)", k, (long long)steps);
    if (S.touch_mode && (S.n_multi < 0 || S.n_multi > S.n_active)) return fail(-1, "ure_job_create: shard %d: n_multi outside [0, n_active]", k);
    if (tag_partitioned(S.N) && !(S.inv_stage && S.inv_off)) return fail(-1, "ure_job_create: shard %d lacks inv_stage / inv_off", k);
    return 0;
}

static bool snapshot_set_ok(const ure_shard_t &S)
{
    const bool full = S.snapU && S.snapV && !S.snap, compact = S.snap && !S.snapU && !S.snapV && S.lazy_rows;
    return !(S.snapU || S.snapV || S.snap) || ((full || compact) && (!S.lazy_rows || S.snap_a));
}

// The optimizer (struct ure_shard: optimizer): every shard of a job the same.  Adam has no closed form for rows without interactions, so
// nothing that rests on one goes with it.  Why shard k may not have what it asks for, or nullptr.
static const char *optimizer_refusal(const ure_shard_t *shards, int k)
{
    const ure_shard_t &S = shards[k];
    if (S.optimizer != 0 && S.optimizer != 1) return "optimizer is 0 (SGD with momentum) or 1 (Adam)";
    if (S.optimizer != shards[0].optimizer) return "every shard of a job must ask for the same optimizer";
    if (S.optimizer == 0) return nullptr;
    if (!S.vU || !S.vV) return "Adam needs the second-moment tables vU and vV";
    if (!S.opt_sc) return "Adam needs the per-step scalars opt_sc";
    if (!(S.beta1 >= 0.f && S.beta1 < 1.f) || !(S.beta2 >= 0.f && S.beta2 < 1.f)) return "Adam needs beta1 and beta2 in [0, 1)";
    if (!(S.eps > 0.f)) return "Adam needs eps > 0";
    if (S.touch_mode) return "Adam does not go with touch_mode (rows between their own steps have no closed form)";
    if (S.snap) return "Adam does not go with compact snapshots (snap): full ones, snapU + snapV";
    if (S.lazy_rows) return "Adam does not go with lazy_rows (rows without interactions have no closed form: they are streamed every step)";
    return nullptr;
}

// touch mode: all shards of the job or none, all in the same mode and on the same optimizer schedule (one closed-form table per job).
// Why shard k may not have it, or nullptr; `steps` = its steps per epoch (valid descriptors only).
static const char *touch_refusal(const ure_shard_t *shards, int k, int steps)
{
    const ure_shard_t &S = shards[k], &S0 = shards[0];
    if (!S.touch_mode) return "every shard of a job must ask for it";
    if (S.touch_mode < 1 || S.touch_mode > 3) return "touch_mode is 0, 1, 2 or 3";
    if (S.touch_mode != S0.touch_mode) return "every shard of a job must ask for the same touch mode";
    if (S.touch_mode == 2 && steps > kAheadMaxSteps) return "touch_mode 2 takes at most 63 steps per epoch (the mask word's top bit is the start buffer)";
    if (S.touch_mode == 2 && (S.snapU || S.snapV)) return "touch_mode 2 writes compact snapshots only (snap + row_slot)";
    if (S.touch_mode == 2 && S.snap && !S.row_slot) return "touch_mode 2 needs row_slot with snap";
    if (S.touch_mode == 3 && steps > kIdxMaxSteps) return "touch_mode 3 takes at most 1008 steps per epoch (16 mask words of 63 steps)";
    if (S.touch_mode == 3 && (S.n_multi > kIdxHeavyMax || S.n_split < 0 || S.n_split > S.n_multi)) return "touch_mode 3: 0 <= n_split <= n_multi <= 256";
    if (S.touch_mode == 3 && S.batch > 200000) return "touch_mode 3 takes batches of at most 200,000 (the parts of a split row are numbered in 11 bits)";
    if (!S.lazy_rows) return "it needs lazy_rows";
    if (steps > kTouchMaxSteps) return "more than 32000 steps per epoch (the step number shares the 16-bit batch tag with the buffer bit)";
    // (both shards have lazy_rows here, hence an lr_host of `epochs` entries each)
    if (S.epochs != S0.epochs || S.lam != S0.lam || S.mu != S0.mu || !std::equal(S.lr_host, S.lr_host + S.epochs, S0.lr_host)) return "the shards' optimizer schedules differ";
    return nullptr;
}

// Every check of ure_job_create, in the order its messages have always come: descriptors shard by shard, (the optimizer,) then snapshot sets, then touch mode.
static int check_shards(const ure_shard_t *shards, int n_shards)
{
    bool touch = false;
    for (int k = 0; k < n_shards; ++k) {
        if (int rc = check_descriptor(shards, k)) return rc;
        touch = touch || shards[k].touch_mode != 0;
    }
    for (int k = 0; k < n_shards; ++k)
        if (const char *why = optimizer_refusal(shards, k)) return fail(-1, "ure_job_create: optimizer refused for shard %d: %s", k, why);
    for (int k = 0; k < n_shards; ++k)
        if (!snapshot_set_ok(shards[k])) return fail(-1, "ure_job_create: shard %d has an incomplete snapshot set (full: snapU + snapV; compact: snap with lazy_rows; snap_a with lazy_rows)", k);
    for (int k = 0; k < n_shards && touch; ++k)
        if (const char *why = touch_refusal(shards, k, make_shard_aux(shards[k]).steps)) return fail(-1, "ure_job_create: touch mode refused for shard %d: %s", k, why);
    return 0;
}

// ---- the plan: per-shard derived constants, the job-wide maxima the launches size their grids by, and the switches

static void plan_job(ure_job *job, const ure_shard_t *shards, int n_shards)
{
    job->host.assign(shards, shards + n_shards);
    job->d = shards[0].d;
    if (const char *e = std::getenv("URE_SHARD_FAST")) { job->shard_fast = e[0] != '0'; job->shard_sliced = e[0] == '2'; }
    if (const char *e = std::getenv("URE_INDEX_STAGED")) job->scatter_staged = e[0] != '0';
    job->adam = shards[0].optimizer == 1;
    job->ahead = shards[0].touch_mode == 2;
    job->index = shards[0].touch_mode == 3;
    for (int k = 0; k < n_shards; ++k) {
        const ure_shard_t &S = shards[k];
        const shard_aux A = make_shard_aux(S);
        const int n_rows = S.n_user + S.n_item, per_block = kBlock / lanes_per_row(S.d);
        job->aux_host.push_back(A);
        job->lr_host.emplace_back(S.lr_host ? std::vector<float>(S.lr_host, S.lr_host + S.epochs) : std::vector<float>());
        job->host[k].lr_host = nullptr;                       // the caller's array need not outlive this call
        job->ticks = std::max(job->ticks, (int64_t)A.steps * S.epochs);
        job->row_blocks.push_back(S.touch_mode ? S.n_units / per_block + (S.n_active - S.n_multi + kBlock - 1) / kBlock      // units + candidate workgroups
                                               : S.n_units / per_block + (S.lazy_rows ? 0 : (n_rows - S.n_active + per_block - 1) / per_block));
        job->max_n = std::max(job->max_n, S.N);
        job->max_slots = std::max(job->max_slots, S.n_slots);
        const bool small = tag_partitioned(S.N);
        (small ? job->small_shards : job->large_shards) = true;
        if (small) job->max_small_n = std::max(job->max_small_n, S.N);
        job->max_lazy = std::max<int64_t>(job->max_lazy, S.lazy_rows ? (int64_t)(n_rows - S.n_active) * (S.d / 4) : 0);
        if (S.snapU || S.snap) {
            job->snapshots = true;
            const int64_t rows = S.snap ? S.n_active : n_rows;      // compact : full
            job->snap_blocks = std::max<unsigned>(job->snap_blocks, (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows * (S.d / 4) + kBlock - 1) / kBlock, 2048)));
        }
        job->all_file_tags = job->all_file_tags && S.file_tags != nullptr;
        if (S.touch_mode) {
            job->touch = true;
            job->index_split = job->index_split || (job->index && S.n_split > 0);
            job->max_units = std::max(job->max_units, S.n_units);
            job->max_active4 = std::max<int64_t>(job->max_active4, (int64_t)S.n_active * (S.d / 4));
            job->max_rows = std::max(job->max_rows, n_rows);
        }
    }
}

// ---- touch mode: the closed-form table and the library-owned device memory

// A_e^j for j = 0 .. tab_n - 1 optimizer steps without a gradient at every epoch's learning rate, in double: (w, m)' = A (w, m),
// m' = mu m + lam w, w' = w - lr m'
static std::vector<float> closed_form_table(const ure_job *job, int tab_n)
{
    const int E = job->host[0].epochs;
    std::vector<float> tab((size_t)E * tab_n * 4);
    const double lam = (double)job->host[0].lam, mu = (double)job->host[0].mu;
    for (int ep = 0; ep < E; ++ep) {
        const double lr = (double)job->lr_host[0][(size_t)ep];
        const double a11 = 1.0 - lr * lam, a12 = -lr * mu, a21 = lam, a22 = mu;
        double p11 = 1.0, p12 = 0.0, p21 = 0.0, p22 = 1.0;
        for (int j = 0; j < tab_n; ++j) {
            float *o = &tab[((size_t)ep * tab_n + j) * 4];
            o[0] = (float)p11; o[1] = (float)p12; o[2] = (float)p21; o[3] = (float)p22;
            const double q11 = a11 * p11 + a12 * p21, q12 = a11 * p12 + a12 * p22;
            const double q21 = a21 * p11 + a22 * p21, q22 = a21 * p12 + a22 * p22;
            p11 = q11; p12 = q12; p21 = q21; p22 = q22;
        }
    }
    return tab;
}

// One block of library-owned device memory: taken from the cache, recorded in the job (ure_job_destroy gives it back) and, as a block
// of the cache comes with whatever its last job left in it, filled with the byte `fill` (kNoFill: the caller writes it).
constexpr int kNoFill = -1;
template <class T>
static hipError_t job_block(ure_job *job, size_t bytes, int fill, T **out)
{
    void *p = nullptr;
    const hipError_t e = block_malloc(&p, bytes);
    if (e != hipSuccess) return e;
    job->touch_mem.push_back(p);
    *out = static_cast<T *>(p);
    return fill == kNoFill ? hipSuccess : hipMemset(p, fill, bytes);
}

// touch_mode 3: the arrays of a shard's slot index (mf_index.h) in one block, each on a 256-byte boundary.  Walked twice: from a null
// base for the size of the block, then from the block.
struct Carve {
    uintptr_t base;
    size_t at = 0;
    template <class T>
    void take(T *&p, size_t bytes) { p = reinterpret_cast<T *>(base + at); at += (bytes + 255) / 256 * 256; }
};
static size_t carve_index(shard_aux &A, const ure_shard_t &S, void *base)
{
    const size_t n_all = (size_t)S.n_user + S.n_item, steps = (size_t)A.steps, slots = (size_t)S.n_slots, hw = (size_t)A.idx_hw;
    const size_t items = (size_t)std::min<int64_t>(2 * (int64_t)S.N, S.n_slots) + 1;
    Carve c{reinterpret_cast<uintptr_t>(base)};
    c.take(A.grp_row, slots / 8 * 8);
    c.take(A.W, (size_t)A.idx_words * n_all * 8);                 // from here ...
    c.take(A.end_par[0], 2 * n_all);
    c.take(A.first_step, n_all * 2 + (size_t)A.idx_words * n_all * 2);
    c.take(A.hist, (size_t)A.idx_chunks * (steps + 1) * 4);       // ... to here a job starts from zeros: masks, end-of-epoch buffers, first steps
    c.take(A.seg, (size_t)kIdxSeg * (steps + 1) * 4);
    c.take(A.step_begin, (steps + 2) * 4);
    c.take(A.sslot, slots * 16);
    c.take(A.runflag, (slots / 64 + 2) * 8);
    c.take(A.blk_cnt, (slots / kIdxFlagBlock + 2) * 4);
    c.take(A.items, items * 16);
    c.take(A.step_item, (steps + 2) * 4);
    c.take(A.heavy_cnt, steps * 4);
    c.take(A.items2, items * 16);
    c.take(A.heavy_cum, steps * (kIdxHeavyMax + 1) * 4);
    c.take(A.partial, hw * (S.d + 4) * 4);
    c.take(A.heavy_map, steps * hw * 4);
    c.take(A.heavy_wg, steps * 4);
    c.take(A.step_desc, steps * 16);
    A.end_par[1] = A.end_par[0] + n_all;
    A.next_first = A.first_step + n_all;
    return c.at;
}

static hipError_t index_memory(ure_job *job, int k, const float4 *ptab, bool index_short)
{
    const ure_shard_t &S = job->host[k];
    shard_aux &A = job->aux_host[k];
    A.ptab = ptab;
    A.idx_words = (int32_t)(((size_t)A.steps + kIdxWin - 1) / kIdxWin);
    A.idx_chunk = index_short ? kIdxStage : kIdxChunk;
    A.idx_chunks = (int32_t)(((size_t)S.n_slots + A.idx_chunk - 1) / A.idx_chunk);
    A.idx_hw = S.n_multi + 2 * S.batch / kIdxPart + 2;
    A.idx_light = (int32_t)std::min<int64_t>(2 * (int64_t)S.batch, S.n_active);
    char *mem = nullptr;
    if (hipError_t e = job_block(job, carve_index(A, S, nullptr), kNoFill, &mem)) return e;
    carve_index(A, S, mem);
    return hipMemset(A.W, 0, (size_t)(reinterpret_cast<char *>(A.hist) - reinterpret_cast<char *>(A.W)));
}

// touch_mode 1 and 2: the row masks of both window parities, the same in work order, and what each mode adds to them
static hipError_t window_memory(ure_job *job, int k, const float4 *ptab)
{
    using mask_t = unsigned long long;
    const ure_shard_t &S = job->host[k];
    shard_aux &A = job->aux_host[k];
    A.ptab = ptab;
    const size_t n_all = (size_t)(S.n_user + S.n_item);
    if (hipError_t e = job_block(job, 2 * n_all * sizeof(mask_t), 0, &A.mask[0])) return e;
    A.mask[1] = A.mask[0] + n_all;
    // the masks once more in work order: per work unit (multi-pass rows) and per single-pass row of the schedule
    const size_t n_um = (size_t)std::max(S.n_units, 1), n_sm = (size_t)std::max(S.n_active - S.n_multi, 1);
    if (hipError_t e = job_block(job, (2 * n_um + n_sm) * sizeof(mask_t), 0, &A.unit_mask)) return e;
    A.unit_own = A.unit_mask + n_um;
    A.sched_mask = A.unit_mask + 2 * n_um;
    A.n_um = (int32_t)n_um;
    A.n_sm = (int32_t)n_sm;
    if (!job->ahead && A.windows > 1 && S.n_units > 0) {
        // epochs of several windows: the steps of every scan pass of the multi-pass units (mf_touch.h: pass skipping)
        if (hipError_t e = job_block(job, ((size_t)S.n_slots / 8 + 1) * sizeof(mask_t), 0, &A.pass_mask)) return e;
    }
    if (job->ahead) {
        // touch_mode 2: the work-order masks once per epoch parity (the first set is the one above), and the owners' hand-over
        A.ahead_masks[0] = A.unit_mask;
        if (hipError_t e = job_block(job, (2 * n_um + n_sm) * sizeof(mask_t), 0, &A.ahead_masks[1])) return e;
        if (hipError_t e = job_block(job, n_um + n_sm, 0xFF, &A.unit_nf)) return e;
        A.sched_nf = A.unit_nf + n_um;
    }
    return hipSuccess;
}

static hipError_t touch_memory(ure_job *job)
{
    int tab_n = kTouchTab;                                      // a window's 64 steps; touch_mode 3: a row may wait a whole epoch for its next step
    if (job->index)
        for (const shard_aux &A : job->aux_host) tab_n = std::max(tab_n, A.steps + 1);
    for (shard_aux &A : job->aux_host) A.ptab_stride = tab_n;
    const std::vector<float> tab = closed_form_table(job, tab_n);
    float4 *ptab = nullptr;
    if (hipError_t e = job_block(job, tab.size() * sizeof(float), kNoFill, &ptab)) return e;
    if (hipError_t e = hipMemcpy(ptab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice)) return e;
    // (epochs of at most 63 steps in every shard: idx_scatter_short_kernel sorts 1,024 slots at a time in LDS, and with a chunk of that size a
    // wavefront per 1,024 slots instead of 4,096 -- the shards of such a job start their epochs at different ticks, 25 / 26 / 27 steps apart, and a
    // single shard's 340 chunks of 4,096 left three quarters of the chip idle: 100 us per shard and epoch against 26 with all 32 at once)
    bool index_short = true;
    for (const shard_aux &A : job->aux_host) index_short = index_short && A.steps <= kIdxWin;
    for (int k = 0; k < (int)job->host.size(); ++k)
        if (hipError_t e = job->index ? index_memory(job, k, ptab, index_short) : window_memory(job, k, ptab)) return e;
    return hipSuccess;
}

static hipError_t upload_job(ure_job *job)
{
    const size_t n = job->host.size();
    if (hipError_t e = hipMalloc(&job->dev, sizeof(ure_shard_t) * n)) return e;
    if (hipError_t e = hipMemcpy(job->dev, job->host.data(), sizeof(ure_shard_t) * n, hipMemcpyHostToDevice)) return e;
    if (hipError_t e = hipMalloc(&job->dev_ab, sizeof(double) * 2 * n)) return e;
    if (job->touch)
        if (hipError_t e = touch_memory(job)) return e;
    if (hipError_t e = hipMalloc(&job->dev_aux, sizeof(shard_aux) * n)) return e;
    return hipMemcpy(job->dev_aux, job->aux_host.data(), sizeof(shard_aux) * n, hipMemcpyHostToDevice);
}

}  // namespace ure

extern "C" int ure_job_create(const ure_shard_t *shards, int n_shards, ure_job_t **out)
{
    URE_ARG(shards && out && n_shards > 0 && n_shards <= 65535);
    if (int rc = ure::check_shards(shards, n_shards)) return rc;
    auto *job = new ure::ure_job();
    std::unique_ptr<ure_job_t, decltype(&ure_job_destroy)> hold(reinterpret_cast<ure_job_t *>(job), ure_job_destroy);
    ure::plan_job(job, shards, n_shards);
    const hipError_t e = ure::upload_job(job);
    if (e != hipSuccess && ure::block_fill_setting(nullptr) < 0)
        return ure::fail(-1, "ure_job_create: URE_BLOCK_FILL='%s' is not a byte (0 .. 255, decimal or 0x..): no block was handed out", std::getenv("URE_BLOCK_FILL"));
    if (e != hipSuccess) return ure::fail((int)e, "ure_job_create: %s", hipGetErrorString(e));
    *out = hold.release();
    return 0;
}

extern "C" int ure_job_destroy(ure_job_t *j)
{
    auto *job = reinterpret_cast<ure::ure_job *>(j);
    if (!job) return 0;
    if (job->dev) (void)hipFree(job->dev);
    if (job->dev_ab) (void)hipFree(job->dev_ab);
    if (job->dev_aux) (void)hipFree(job->dev_aux);
    for (void *p : job->touch_mem) ure::block_free(p);          // (the three frees above have waited for the device)
    delete job;
    return 0;
}
