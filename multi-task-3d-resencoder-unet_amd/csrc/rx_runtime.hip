// rx_runtime.hip -- host state of the library: the per-thread error string, the note of which kernel instantiation the last
// conv entry point used (and its sequence number, which rx_prog.hip reads), the ABI version and the architecture check.
#include <stdarg.h>

#include "rx_common.h"
#include "rx_internal.h"

// ---------------------------------------------------------------------------------------------
// error string
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void rx_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* rx_last_error(void) { return g_err; }
static thread_local const char* g_last_kernel = "";
static thread_local int g_note_seq_ = 0;
void rx_note_kernel(const char* name) { g_last_kernel = name; ++g_note_seq_; }
int rx_note_seq(void) { return g_note_seq_; }
extern "C" const char* rx_last_conv_kernel(void) { return g_last_kernel; }
extern "C" int rx_abi_version(void) { return 1; }
extern "C" int rx_device_arch_ok(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
  return strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}
