// exact.h -- what the host drivers (tests/host_drivers/*.inc) share: the exact-size allocation and the opening, reading
// and closing of a driver's two files.
#pragma once

#include <cstddef>
#include <cstdio>
#include <cstdlib>

namespace host {

// A driver's exit status where IN or OUT cannot be opened, IN is short or holds a value out of range, or OUT cannot be
// written whole.
constexpr int kBadInput = 2;

// An allocation of exactly count * sizeof(T) bytes: an access one element past it is a sanitizer report.  It is aligned
// as malloc aligns, or to Align where a driver asks for more (posix_memalign takes any size, so nothing is rounded up).
// Count 0 is a null pointer, the stricter choice: nothing may be read or written through it, and `read` / `write` pass
// no null pointer to fread / fwrite.
template <class T, size_t Align = alignof(T)>
struct Exact {
  T* p = nullptr;
  size_t n;
  explicit Exact(size_t count) : n(count) {
    constexpr size_t align = Align > alignof(max_align_t) ? Align : alignof(max_align_t);
    void* v = nullptr;
    if (count && posix_memalign(&v, align, count * sizeof(T)) != 0) abort();
    p = static_cast<T*>(v);
  }
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
  bool read(FILE* f) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
  bool write(FILE* f, size_t count) const { return count == 0 || fwrite(p, sizeof(T), count, f) == count; }
  bool write(FILE* f) const { return write(f, n); }
  void fill(T v) { for (size_t i = 0; i < n; ++i) p[i] = v; }
};

// A driver's arguments are NAME IN OUT [flags ...]: opens IN for reading and OUT for writing.
inline bool open_files(int argc, char** argv, FILE** in, FILE** out) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s IN OUT [flags ...]\n", argv[0]);
    return false;
  }
  *in = fopen(argv[1], "rb");
  *out = fopen(argv[2], "wb");
  if (!*in || !*out) fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
  return *in && *out;
}

// One value of a plain type; false on a short read.
template <class T>
bool read_pod(FILE* f, T* v) { return fread(v, sizeof(T), 1, f) == 1; }

// The driver's exit status once every case is written.
inline int close_files(FILE* in, FILE* out) {
  fclose(in);
  return fclose(out) == 0 ? 0 : kBadInput;
}

}  // namespace host
