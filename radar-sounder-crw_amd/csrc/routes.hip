// The route log (include/crw_hip_routes.h): the table behind CRW_ROUTE (crw_common.h).  Host code only.
#include "crw_common.h"
#include "crw_hip_routes.h"

#include <fcntl.h>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

namespace crw {
namespace {

RouteSite g_sites[MAX_ROUTES + 1];   // the last slot takes every name past a full table (its counts are meaningless, never lost writes)
std::atomic<int> g_nsites{0};        // published after the slot's name is written
std::mutex g_register;

void log_name(const char *name) {
  const char *path = getenv("CRW_ROUTE_LOG");
  if (!path || !path[0]) return;
  const int fd = open(path, O_WRONLY | O_APPEND | O_CREAT, 0644);
  if (fd < 0) return;
  char line[128];
  const size_t len = strnlen(name, sizeof(line) - 1);
  memcpy(line, name, len);
  line[len] = '\n';
  (void)!write(fd, line, len + 1);   // one write per line: O_APPEND keeps lines of concurrent processes whole
  close(fd);
}

}  // namespace

// Called once per site (the site's function-local static): a name registers once however many sites (template instances) pass it.
RouteSite *route_register(const char *name) {
  std::lock_guard<std::mutex> lock(g_register);
  const int n = g_nsites.load(std::memory_order_relaxed);
  for (int i = 0; i < n; ++i)
    if (!strcmp(g_sites[i].name, name)) return &g_sites[i];
  if (n == MAX_ROUTES) return &g_sites[MAX_ROUTES];
  g_sites[n].name = name;
  g_nsites.store(n + 1, std::memory_order_release);
  log_name(name);
  return &g_sites[n];
}

}  // namespace crw

extern "C" int crw_routes_clear(void) {
  const int n = crw::g_nsites.load(std::memory_order_acquire);
  for (int i = 0; i < n; ++i) crw::g_sites[i].count.store(0, std::memory_order_relaxed);
  return CRW_OK;
}

extern "C" int crw_routes_read(const char **names, long *counts, int max) {
  const int n = crw::g_nsites.load(std::memory_order_acquire);
  for (int i = 0; i < n && i < max; ++i) {
    if (names) names[i] = crw::g_sites[i].name;
    if (counts) counts[i] = crw::g_sites[i].count.load(std::memory_order_relaxed);
  }
  return n;
}
