// pgtt_side_host.h — the host prelude of every side library (libpgtt_render.so, _depth, _perceive, _elevation, _learn, _lidar): the thread-local error
// string, the check of the device index, and the two exports they all have, pgtt_<x>_last_error() and pgtt_<x>_build_info().  Everything but the
// two exports is in an anonymous namespace: each library keeps its own error string and exports nothing of this.  `who` is the entry point's
// name, the prefix of its messages.  No device code here.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pgtt.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) return fail(PGTT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

int check_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PGTT_E_NODEVICE, std::string(who) + ": no HIP device (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(PGTT_E_ARG, std::string(who) + ": device index out of range");
  return PGTT_OK;
}

// `text` is a macro's name put through PGTT_SIDE_STR: "\"value\"" when the macro is defined as a string literal, its own name when it is not
// defined - which is how one macro can hold the defaults of six pairs of names
std::string literal_or(const char* text, const char* otherwise) {
  const std::string s(text);
  return s.size() >= 2 && s.front() == '"' ? s.substr(1, s.size() - 2) : otherwise;
}

std::string build_info(const char* src, const char* flavor) {
  std::string info("src=");
  info += literal_or(src, "unknown");
  info += ";flavor=";
  info += literal_or(flavor, "product");
  return info;
}

}  // namespace

#define PGTT_SIDE_STR_(x) #x
#define PGTT_SIDE_STR(x) PGTT_SIDE_STR_(x)

// PGTT_SIDE_EXPORTS(depth, DEPTH) defines pgtt_depth_last_error() and pgtt_depth_build_info() = "src=<PGTT_DEPTH_SRC>;flavor=<PGTT_DEPTH_FLAVOR>":
// the make file gives -DPGTT_DEPTH_SRC=\"<srchash.side_sha256>\" ("unknown" without it), and an experiment build names itself with
// EXTRA='-DPGTT_DEPTH_FLAVOR=\"name\"' ("product" without it); csrc/pgtt_side.mk has the full lines
#define PGTT_SIDE_EXPORTS(x, X)                                                                                                    \
  extern "C" const char* pgtt_##x##_last_error(void) { return g_err.c_str(); }                                                     \
  extern "C" const char* pgtt_##x##_build_info(void) {                                                                             \
    static const std::string info = build_info(PGTT_SIDE_STR(PGTT_##X##_SRC), PGTT_SIDE_STR(PGTT_##X##_FLAVOR));                   \
    return info.c_str();                                                                                                           \
  }
