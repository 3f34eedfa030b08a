// corb_scratch.cpp -- the C-ABI calls on the per-device workspace lanes themselves (corb_workspace.h): warm-up, release, and the dense SPD solve that runs in one.
#include "ba_host.h"
#include "dense_chol.h"

extern "C" int corb_warmup(int device)
{
    int rc = corb_select_device(device); if (rc) return rc;
    // Rounds 1-2 ran rocSOLVER's factorisations once here, because rocBLAS / rocSOLVER load their kernel libraries lazily (seconds inside the first
    // optimisation of a process).  The library links neither any more: what is left to warm up are the two workspace lanes (stream, events, pinned block).
    for (int lane = 0; lane < 2; lane++) {
        CorbScratch pool(lane);
        if (!pool.stream) { corb_set_error("corb_warmup: workspace creation failed"); return CORB_ERR_HIP; }
    }
    return CORB_OK;
}

// Device and page-locked memory the library keeps between calls goes back to the runtime: the arenas of the device's two workspace lanes and the staging of large host-array
// BA calls.  A lane (or the staging) that a call of another thread holds at this moment is left alone.  The next call that needs them allocates them again.
extern "C" int corb_release_scratch(int device, uint64_t* bytes_released)
{
    int rc = corb_select_device(device); if (rc) return rc;
    uint64_t freed = 0;
    for (int lane = 0; lane < 2; lane++) {
        CorbWorkspace& ws = corb_workspace(device, lane);
        std::unique_lock<std::mutex> lk(ws.mu, std::try_to_lock);
        if (!lk.owns_lock()) continue;
        if (ws.stream) (void)hipStreamSynchronize(ws.stream);
        for (auto& c : ws.chunks) { freed += c.cap; (void)hipFree(c.base); }
        ws.chunks.clear();
        if (ws.hstage) { freed += ws.hcap; (void)hipHostFree(ws.hstage); ws.hstage = nullptr; ws.hcap = 0; ws.hused = 0; ws.hwant = 0; }
    }
    freed += ba_host_fast_release(device);
    if (bytes_released) *bytes_released = freed;
    return CORB_OK;
}

// Test aids on a lane's arena (the rule they let a test check: every byte a call reads from the arena or the staging was written earlier in the same call).
// None of them is part of a call's work: they only put the lane into a known state between calls and look at it afterwards.
// corb_scratch_fill fills whole 32-bit words: every chunk's capacity is a multiple of 256 bytes (CorbWorkspace::take rounds, reset() adds such sizes up).  If the
// one new chunk cannot be allocated, the call fails with the arena left empty, as after corb_release_scratch: the next call allocates it again.
extern "C" int corb_scratch_fill(int device, int lane, uint32_t word, uint64_t min_bytes, uint64_t* capacity)
{
    if (lane < 0 || lane > 1) { corb_set_error("corb_scratch_fill: lane must be 0 or 1"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    CorbWorkspace& ws = corb_workspace(device, lane);
    std::unique_lock<std::mutex> lk(ws.mu);
    HIPCHK(ws.ensure());
    HIPCHK(hipStreamSynchronize(ws.stream));
    size_t total = 0; for (auto& c : ws.chunks) total += c.cap;
    const size_t want = std::max(total, (((size_t)min_bytes + 255) & ~(size_t)255));
    if (ws.chunks.size() != 1 || ws.chunks[0].cap < want) {
        for (auto& c : ws.chunks) (void)hipFree(c.base);
        ws.chunks.clear();
        if (want) { void* p = nullptr; HIPCHK(hipMalloc(&p, want)); ws.chunks.push_back({(char*)p, want, 0}); }
    }
    for (auto& c : ws.chunks) { c.used = 0; HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c.base, (int)word, c.cap / 4, ws.stream)); }
    HIPCHK(hipStreamSynchronize(ws.stream));
    if (ws.hstage) std::fill((uint32_t*)ws.hstage, (uint32_t*)ws.hstage + ws.hcap / 4, word);
    std::fill((uint32_t*)ws.pinned, (uint32_t*)ws.pinned + 4096 / 4, word);
    if (capacity) *capacity = want;
    return CORB_OK;
}

extern "C" int corb_scratch_report(int device, int lane, uint64_t* capacity, int* n_chunks, uint64_t* staging_capacity)
{
    if (lane < 0 || lane > 1) { corb_set_error("corb_scratch_report: lane must be 0 or 1"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    CorbWorkspace& ws = corb_workspace(device, lane);
    std::unique_lock<std::mutex> lk(ws.mu);
    size_t total = 0; for (auto& c : ws.chunks) total += c.cap;
    if (capacity) *capacity = total;
    if (n_chunks) *n_chunks = (int)ws.chunks.size();
    if (staging_capacity) *staging_capacity = ws.hstage ? ws.hcap : 0;
    return CORB_OK;
}

extern "C" int corb_scratch_read(int device, int lane, uint64_t offset, uint64_t bytes, void* out)
{
    if (lane < 0 || lane > 1 || (bytes && !out)) { corb_set_error("corb_scratch_read: bad argument"); return CORB_ERR_ARG; }
    int rc = corb_select_device(device); if (rc) return rc;
    CorbWorkspace& ws = corb_workspace(device, lane);
    std::unique_lock<std::mutex> lk(ws.mu);
    if (ws.chunks.size() != 1) { corb_set_error("corb_scratch_read: the arena is not one chunk"); return CORB_ERR_ARG; }
    if (offset > ws.chunks[0].cap || bytes > ws.chunks[0].cap - offset) { corb_set_error("corb_scratch_read: range beyond the arena"); return CORB_ERR_ARG; }
    if (ws.stream) HIPCHK(hipStreamSynchronize(ws.stream));
    if (bytes) HIPCHK(hipMemcpy(out, ws.chunks[0].base + offset, (size_t)bytes, hipMemcpyDeviceToHost));
    return CORB_OK;
}

extern "C" int corb_spd_solve(const double* A, int n, const double* b, double* x, int* info, int device)
{
    if (n < 0 || (n > 0 && (!A || !b || !x))) { corb_set_error("corb_spd_solve: bad argument"); return CORB_ERR_ARG; }
    if (info) *info = 0;
    if (n == 0) return CORB_OK;
    int rc = corb_select_device(device); if (rc) return rc;
    CorbScratch pool(0);
    double *dA, *db; int* dinfo;
    HIPCHK(pool.alloc(&dA, (size_t)n * n)); HIPCHK(pool.alloc(&db, (size_t)n)); HIPCHK(pool.alloc(&dinfo, 1));
    HIPCHK(hipMemcpyAsync(dA, A, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, pool.stream));
    HIPCHK(hipMemcpyAsync(db, b, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, pool.stream));
    double* dws; HIPCHK(pool.alloc(&dws, corb_chol_workspace_doubles(n)));
    corb_launch_chol_solve(dA, n, n, db, dinfo, dws, pool.stream);
    HIPCHK(hipGetLastError());
    int h_info = 0;
    HIPCHK(hipMemcpyAsync(x, db, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, pool.stream));
    HIPCHK(hipMemcpyAsync(&h_info, dinfo, sizeof(int), hipMemcpyDeviceToHost, pool.stream));
    HIPCHK(hipStreamSynchronize(pool.stream));
    if (info) *info = h_info;
    return CORB_OK;
}
