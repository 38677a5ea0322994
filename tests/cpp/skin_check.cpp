// skin_check -- skin_mesh_host() of csrc/prt_skin.h (the code the skinning kernels run per vertex and per primitive)
// over arrays read from files, for tests/test_skin_ref.py.  Plain C++, no HIP.
//
//   skin_check V T J positions normals indices joints weights uvs matrices out_prefix
//
// reads raw little-endian arrays (float32; indices int32, joints uint16; uvs 6 per triangle) and writes the six arrays
// of a prt_mesh to out_prefix.triangles / .fixed_normals / .fixed_uvs / .indices / .vertices / .face_normals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "prt_skin.h"

template <class T>
static bool read_file(const char* path, std::vector<T>& out, size_t n) {
  out.resize(n);
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t got = std::fread(out.data(), sizeof(T), n, f);
  const bool end = std::fgetc(f) == EOF;
  std::fclose(f);
  return got == n && end;
}

template <class T>
static bool write_file(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t put = std::fwrite(v.data(), sizeof(T), v.size(), f);
  return std::fclose(f) == 0 && put == v.size();
}

int main(int argc, char** argv) {
  if (argc != 12) {
    std::fprintf(stderr, "usage: skin_check V T J positions normals indices joints weights uvs matrices out_prefix\n");
    return 2;
  }
  const long V = std::atol(argv[1]), T = std::atol(argv[2]), J = std::atol(argv[3]);
  if (V < 1 || T < 1 || J < 1 || J > 65536) return 2;
  std::vector<float> P, N, W, UV, M;
  std::vector<int32_t> idx;
  std::vector<uint16_t> jn;
  if (!read_file(argv[4], P, 3 * (size_t)V) || !read_file(argv[5], N, 3 * (size_t)V) ||
      !read_file(argv[6], idx, 3 * (size_t)T) || !read_file(argv[7], jn, 4 * (size_t)V) ||
      !read_file(argv[8], W, 4 * (size_t)V) || !read_file(argv[9], UV, 6 * (size_t)T) ||
      !read_file(argv[10], M, 12 * (size_t)J)) {
    std::fprintf(stderr, "skin_check: an input file is missing or has the wrong size\n");
    return 3;
  }
  for (int32_t i : idx)
    if (i < 0 || i >= V) return 4;
  for (uint16_t j : jn)
    if (j >= J) return 4;
  std::vector<float> tri(12 * (size_t)T), fnrm(12 * (size_t)T), vtx(3 * (size_t)V), face(3 * (size_t)T),
      tmp(3 * (size_t)V);
  prt::skin_mesh_host((int32_t)V, (int32_t)T, P.data(), N.data(), idx.data(), jn.data(), W.data(), M.data(), tri.data(),
                      fnrm.data(), vtx.data(), face.data(), tmp.data());
  const std::string out = argv[11];
  const bool ok = write_file(out + ".triangles", tri) && write_file(out + ".fixed_normals", fnrm) &&
                  write_file(out + ".fixed_uvs", UV) && write_file(out + ".indices", idx) &&
                  write_file(out + ".vertices", vtx) && write_file(out + ".face_normals", face);
  return ok ? 0 : 5;
}
