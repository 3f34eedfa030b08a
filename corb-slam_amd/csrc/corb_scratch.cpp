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
