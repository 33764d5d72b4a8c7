// capi_saipb.cpp -- lrsc_saipb_merge: the hash-guided seed-pair merge (SAIPBSelfCorrectTree) on the device: saipb.hip /
// saipb_device.h.
#include "capi_internal.h"

using namespace lrsc;

extern "C" int lrsc_saipb_merge(lrsc_ctx* ctx, const char* seq, uint64_t seq_len, const lrsc_saipb_seed* seeds, uint32_t n_seeds,
                                const lrsc_saipb_job* jobs, uint32_t n_jobs, lrsc_saipb_result* results, uint64_t* seed_freq,
                                char* out_arena, uint64_t arena_cap, uint64_t* arena_used)
{
    if(!ctx || !arena_used || (!jobs && n_jobs) || (!results && n_jobs) || (!seeds && n_seeds) || (!seq && seq_len)) return fail(LRSC_ERR_ARG, "null");
    *arena_used = 0;
    if(n_jobs == 0) return LRSC_OK;
    std::vector<SaipbSeed> hseeds(n_seeds);
    std::vector<SaipbJob> hjobs(n_jobs);
    std::vector<uint8_t> seed_used(n_seeds, 0);
    for(uint32_t j = 0; j < n_jobs; ++j) {
        const char* why = "";
        const int st = saipb_from_abi(seeds, n_seeds, jobs[j], seq_len, hseeds.data(), hjobs[j], &why);
        if(st != LRSC_OK) return fail(st, std::string("saipb job ") + std::to_string(j) + ": " + why);
        for(uint32_t s = 0; s < jobs[j].n_seeds; ++s) seed_used[jobs[j].seed_first + s] = 1;
    }
    // a seed no job names is never looked at: give it a harmless record (its frequency is reported as 0)
    for(uint32_t s = 0; s < n_seeds; ++s)
        if(!seed_used[s]) hseeds[s] = SaipbSeed{0, 0, 0, 0, -1, 0, 0};
    HIP_TRY(hipSetDevice(ctx->device));

    // ---- the seeds' intervals: what sizes every job's table ------------------------------------------------------------------
    DevBuf<uint8_t>& d_codes = ctx->sp_codes;
    DevBuf<SaipbSeed>& d_seeds = ctx->sp_seeds;
    DevBuf<SaipbSeedInfo>& d_info = ctx->sp_info;
    HIP_TRY(d_codes.reserve(std::max<uint64_t>(seq_len, 1)));
    HIP_TRY(d_seeds.reserve(std::max<uint32_t>(n_seeds, 1)));
    HIP_TRY(d_info.reserve(std::max<uint32_t>(n_seeds, 1)));
    if(seq_len) {
        const int st = upload_and_encode(ctx, seq, seq_len, d_codes.p);
        if(st != LRSC_OK) return st;
    }
    std::vector<SaipbSeedInfo> info(n_seeds);
    if(n_seeds) {
        // only seeds that a job names are searched: compact them
        std::vector<SaipbSeed> live;
        std::vector<uint32_t> live_at;
        for(uint32_t s = 0; s < n_seeds; ++s) if(seed_used[s]) { live.push_back(hseeds[s]); live_at.push_back(s); }
        DevBuf<SaipbSeed>& d_live = ctx->sp_live;
        DevBuf<SaipbSeedInfo>& d_live_info = ctx->sp_live_info;
        HIP_TRY(d_live.reserve(std::max<size_t>(live.size(), 1)));
        HIP_TRY(d_live_info.reserve(std::max<size_t>(live.size(), 1)));
        HIP_TRY(hipMemcpyAsync(d_live.p, live.data(), live.size() * sizeof(SaipbSeed), hipMemcpyHostToDevice, ctx->stream));
        hipError_t e = launch_saipb_seed_info(ctx->fm, d_codes.p, d_live.p, (uint32_t)live.size(), d_live_info.p, ctx->stream);
        if(e != hipSuccess) return hip_fail(e, "saipb_seed_kernel");
        std::vector<SaipbSeedInfo> live_info(live.size());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(live_info.data(), d_live_info.p, live.size() * sizeof(SaipbSeedInfo), hipMemcpyDeviceToHost));
        for(SaipbSeedInfo& si : info) si = SaipbSeedInfo{1, 0, 1, 0, 0};
        for(size_t i = 0; i < live.size(); ++i) info[live_at[i]] = live_info[i];
        HIP_TRY(hipMemcpyAsync(d_seeds.p, hseeds.data(), (size_t)n_seeds * sizeof(SaipbSeed), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_info.p, info.data(), (size_t)n_seeds * sizeof(SaipbSeedInfo), hipMemcpyHostToDevice, ctx->stream));
        if(seed_freq) for(uint32_t s = 0; s < n_seeds; ++s) seed_freq[s] = info[s].freq;
    }

    // ---- plan: every job's slice, chunks under the workspace budget (never a per-job worst case) -----------------------------------
    const uint64_t budget = env_bytes("LRSC_SAIPB_CHUNK_MB", 1024ull << 20, 20);
    const uint64_t job_cap = env_bytes("LRSC_SAIPB_JOB_KB", 256ull << 20, 10);
    std::vector<SaipbJob> run;                       // the jobs that run, in job order
    std::vector<uint32_t> run_at;
    std::vector<std::pair<uint32_t, uint32_t>> chunks;           // [first, end) into run
    std::vector<SaipbOut> outs(n_jobs, SaipbOut{});
    uint64_t ws_used = 0, ws_max = 0, out_total = 0;
    uint32_t chunk_first = 0;
    for(uint32_t j = 0; j < n_jobs; ++j) {
        SaipbJob& job = hjobs[j];
        if(!saipb_plan_job(job, hseeds.data(), info.data())) { outs[j].status = LRSC_SAIPB_HASH_LIMIT; continue; }
        const uint64_t need = saipb_layout(job).total;
        if(need > job_cap) { outs[j].status = LRSC_SAIPB_HASH_LIMIT; continue; }
        if(ws_used && ws_used + need > budget) {
            chunks.emplace_back(chunk_first, (uint32_t)run.size());
            chunk_first = (uint32_t)run.size();
            ws_used = 0;
        }
        job.ws_off = ws_used;
        ws_used += (need + 63) & ~63ull;
        ws_max = std::max(ws_max, ws_used);
        job.out_off = out_total;
        out_total += job.str_cap;
        run.push_back(job);
        run_at.push_back(j);
    }
    if(chunk_first < run.size()) chunks.emplace_back(chunk_first, (uint32_t)run.size());

    // ---- the chunks, back to back on the stream; nothing comes back to the host in between ---------------------------------------
    std::vector<SaipbOut> run_out(run.size());
    std::vector<char> text(out_total);
    if(!run.empty()) {
        DevBuf<SaipbJob>& d_jobs = ctx->sp_jobs;
        DevBuf<SaipbOut>& d_out = ctx->sp_out;
        DevBuf<uint8_t>& d_ws = ctx->sp_ws;
        DevBuf<char>& d_text = ctx->sp_text;
        HIP_TRY(d_jobs.reserve(run.size()));
        HIP_TRY(d_out.reserve(run.size()));
        HIP_TRY(d_ws.reserve(std::max<uint64_t>(ws_max, 64)));
        HIP_TRY(d_text.reserve(std::max<uint64_t>(out_total, 1)));
        HIP_TRY(hipMemcpyAsync(d_jobs.p, run.data(), run.size() * sizeof(SaipbJob), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
        for(const auto& ch : chunks) {
            hipError_t e = launch_saipb_merge(ctx->fm, d_codes.p, d_seeds.p, d_info.p, d_jobs.p + ch.first, ch.second - ch.first, d_ws.p, d_text.p,
                                              d_out.p + ch.first, ctx->stream);
            if(e != hipSuccess) return hip_fail(e, "saipb_merge_kernel");
        }
        HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        ctx->stats[LRSC_K_SAIPB].launches += chunks.size();     // one launch per chunk; the call's chunks are timed as one span
        ctx->stats[LRSC_K_SAIPB].total_ms += ms;
        HIP_TRY(hipMemcpy(run_out.data(), d_out.p, run.size() * sizeof(SaipbOut), hipMemcpyDeviceToHost));
        if(out_total) HIP_TRY(hipMemcpy(text.data(), d_text.p, out_total, hipMemcpyDeviceToHost));
    }
    for(size_t i = 0; i < run.size(); ++i) outs[run_at[i]] = run_out[i];

    uint64_t used = 0;
    std::vector<uint64_t> text_off(n_jobs, 0);
    for(size_t i = 0; i < run.size(); ++i) text_off[run_at[i]] = run[i].out_off;
    for(uint32_t j = 0; j < n_jobs; ++j) {
        const SaipbOut& o = outs[j];
        lrsc_saipb_result& r = results[j];
        std::memset(&r, 0, sizeof(r));
        r.status = (int32_t)o.status;
        if(o.status != LRSC_SAIPB_OK) continue;                  // no numbers for a job that outgrew a capacity
        r.code = o.code; r.steps = o.steps; r.max_used_leaves = o.max_used_leaves; r.n_results = o.n_results; r.hash_entries = o.hash_entries;
        if(o.code != 1) continue;
        r.out_off = used; r.out_len = o.out_len;
        if(out_arena && used + o.out_len <= arena_cap) std::memcpy(out_arena + used, text.data() + text_off[j], o.out_len);
        used += o.out_len;
    }
    *arena_used = used;
    if(used > arena_cap || (!out_arena && used)) return fail(LRSC_ERR_CAPACITY, "merged-sequence arena too small");
    return LRSC_OK;
}
