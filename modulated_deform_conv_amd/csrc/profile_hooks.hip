// profile_hooks.hip -- benchmark hooks (include/mdconv.h: mdconv_profile_*): event pairs around the kernels the host code
// brackets with profile_mark().  Process-wide, guarded so that a threaded host cannot corrupt the event lists.
#include <atomic>
#include <mutex>
#include <vector>

#include "mfma_kernels.hpp"

namespace mdconv {

namespace {
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
struct ProfPair { hipEvent_t a, b; };
constexpr int kProfSlots = 5;   // forward GEMM, backward data GEMM, backward weight GEMM, grad_input gather, coordinate gradients
std::vector<ProfPair> g_prof[kProfSlots];
size_t g_prof_used[kProfSlots] = {0, 0, 0, 0, 0};
const char *g_prof_name[kProfSlots] = {"", "", "", "", ""};
}  // namespace

void profile_mark(int which, bool begin, hipStream_t stream, const char *name) {
  if (!g_prof_on.load(std::memory_order_relaxed) || which < 0 || which >= kProfSlots) return;
  std::lock_guard<std::mutex> lock(g_prof_mu);
  if (name) g_prof_name[which] = name;
  if (begin) {
    if (g_prof_used[which] == g_prof[which].size()) {
      ProfPair p;
      if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return;
      g_prof[which].push_back(p);
    }
    (void)hipEventRecord(g_prof[which][g_prof_used[which]].a, stream);
  } else if (g_prof_used[which] < g_prof[which].size()) {
    (void)hipEventRecord(g_prof[which][g_prof_used[which]].b, stream);
    ++g_prof_used[which];
  }
}

}  // namespace mdconv

using namespace mdconv;

extern "C" {
int mdconv_profile_enable(int on) {
  const int prev = g_prof_on.exchange(on != 0) ? 1 : 0;
  return prev;
}
void mdconv_profile_reset(void) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  for (int i = 0; i < kProfSlots; ++i) g_prof_used[i] = 0;
}
const char *mdconv_profile_name(int which) {
  if (which < 0 || which >= kProfSlots) return "";
  std::lock_guard<std::mutex> lock(g_prof_mu);
  return g_prof_name[which];
}
int mdconv_profile_read(int which, double *total_ms) {
  if (which < 0 || which >= kProfSlots) return 0;
  double tot = 0;
  int n = 0;
  std::lock_guard<std::mutex> lock(g_prof_mu);
  for (size_t i = 0; i < g_prof_used[which]; ++i) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, g_prof[which][i].a, g_prof[which][i].b) == hipSuccess) {
      tot += ms;
      ++n;
    }
  }
  if (total_ms) *total_ms = tot;
  return n;
}
}
