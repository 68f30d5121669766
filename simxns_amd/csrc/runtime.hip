// Library plumbing shared by every unit: the error text, the compute-CU budget of the persistent kernels and the optional
// per-launch event profiler (prof.h).
#include <stdarg.h>
#include <vector>
#include "common.h"
#include "prof.h"

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void simx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* simx_last_error(void) { return g_err; }
extern "C" int simx_version(void) { return 100; }

// ---- compute-CU budget of the persistent kernels (include/simx.h simx_set_compute_cus) --------------------------------
// The persistent GEMMs launch one workgroup per CU (each needs a whole CU's 160 KB of LDS) and give every workgroup a STATIC share
// of the tile list; the wgrad plans fill exactly one round of the chip.  When another kernel holds k CUs for the whole launch -- an
// RCCL ring during the overlapped backward -- k of those workgroups only start when a resident one has finished its WHOLE share:
// the launch takes up to twice as long (tools/cu_steal_bench, profiles/r06_cu_steal.json).  With a budget of ncu - k the launches
// fit beside the communication kernel and lose k / ncu instead.  0 = every CU (default; SIMX_COMPUTE_CUS until the first explicit set).
static std::atomic<int> g_compute_cus{-1};      // -1: no explicit set yet, the environment's value holds
extern "C" int simx_set_compute_cus(int n) {
  SIMX_REQUIRE(n >= 0, SIMX_ERR_BAD_SHAPE, "simx_set_compute_cus: %d", n);
  g_compute_cus.store(n, std::memory_order_relaxed);
  return SIMX_OK;
}
int simx_compute_cus(int device_cus) {
  static const int env_cus = [] { const char* e = getenv("SIMX_COMPUTE_CUS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 0; }();
  const int set = g_compute_cus.load(std::memory_order_relaxed);
  const int budget = set < 0 ? env_cus : set;
  int n = budget > 0 && budget < device_cus ? budget : device_cus;
  n -= n % 8;                                   // whole XCD rows: xcd_remap assumes block b -> XCD b % 8
  return n < 8 ? 8 : n;
}

// ------------------------------------------------------------------------------------------ profiler
namespace {
struct ProfRec { int id; double work; hipEvent_t a, b; bool done; };
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_pool;
size_t g_pool_next = 0;
}  // namespace

int simx_prof_mark(int id, hipStream_t s, double work, int end_index) {
  if (end_index < 0) {
    if (!g_prof_on || g_pool_next + 2 > g_pool.size()) return -1;
    ProfRec r{id, work, g_pool[g_pool_next], g_pool[g_pool_next + 1], false};
    g_pool_next += 2;
    (void)hipEventRecord(r.a, s);
    g_prof.push_back(r);
    return (int)g_prof.size() - 1;
  }
  if ((size_t)end_index < g_prof.size() && !g_prof[end_index].done) {      // (scopes nest: each closes its own record)
    (void)hipEventRecord(g_prof[end_index].b, s);
    g_prof[end_index].done = true;
  }
  return end_index;
}

void simx_prof_retag(int id) {
  if (!g_prof_on) return;
  for (size_t i = g_prof.size(); i-- > 0;)
    if (!g_prof[i].done) { g_prof[i].id = id; return; }
}

extern "C" int simx_prof_begin(int max_launches) {
  while ((int)g_pool.size() < 2 * max_launches) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) { simx_set_error("prof_begin: hipEventCreate failed"); return SIMX_ERR_HIP; }
    g_pool.push_back(e);
  }
  g_prof.clear();
  g_pool_next = 0;
  g_prof_on = true;
  return SIMX_OK;
}

// Stops recording, waits for the recorded events and aggregates per kernel class:
// counts[k], total_ms[k], total_work[k] for k < SIMX_K_COUNT (host arrays).
extern "C" int simx_prof_end(int32_t* counts_host, double* total_ms_host, double* total_work_host) {
  g_prof_on = false;
  for (int k = 0; k < SIMX_K_COUNT; ++k) { counts_host[k] = 0; total_ms_host[k] = 0; total_work_host[k] = 0; }
  for (auto& r : g_prof) {
    if (!r.done) continue;
    if (hipEventSynchronize(r.b) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    counts_host[r.id] += 1;
    total_ms_host[r.id] += ms;
    total_work_host[r.id] += r.work;
  }
  g_prof.clear();
  (void)hipGetLastError();      // a failed event query must not surface as the next launch's error
  return SIMX_OK;
}
extern "C" int simx_prof_kernel_count(void) { return SIMX_K_COUNT; }
