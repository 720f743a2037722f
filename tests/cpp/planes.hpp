// Raw planes for the C++ test binaries: a directory of little-endian `<name>.bin` files and a plain-text manifest,
// one line per plane — `name type d0 [d1 [d2]]`, type one of f32 / i32 / u64 — written by the Python test on one
// side and by the binary on the other.  A plane whose file is not exactly as long as its manifest line says is
// refused.  Nothing here knows numpy or the library.
#pragma once
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace planes {

struct plane {
  std::string type;            // "f32", "i32", "u64"
  std::vector<int64_t> dims;   // 1 to 3
  std::vector<char> bytes;
  int64_t elem() const {
    int64_t n = 1;
    for (int64_t d : dims) n *= d;
    return n;
  }
};

inline size_t width(const std::string& type) {
  if (type == "f32" || type == "i32") return 4;
  if (type == "u64") return 8;
  throw std::runtime_error("planes: unknown type " + type);
}

// every plane the manifest `<dir>/<manifest>` lists
inline std::map<std::string, plane> read_all(const std::string& dir, const std::string& manifest) {
  std::ifstream list(dir + "/" + manifest);
  if (!list) throw std::runtime_error("planes: cannot open " + dir + "/" + manifest);
  std::map<std::string, plane> out;
  std::string line;
  while (std::getline(list, line)) {
    if (line.empty()) continue;
    std::istringstream words(line);
    std::string name;
    plane p;
    words >> name >> p.type;
    for (int64_t d; words >> d;) p.dims.push_back(d);
    if (name.empty() || p.dims.empty() || p.dims.size() > 3) throw std::runtime_error("planes: bad line: " + line);
    for (int64_t d : p.dims)
      if (d <= 0) throw std::runtime_error("planes: bad line: " + line);
    const size_t want = static_cast<size_t>(p.elem()) * width(p.type);
    std::ifstream file(dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!file) throw std::runtime_error("planes: cannot open " + name + ".bin");
    if (static_cast<size_t>(file.tellg()) != want)
      throw std::runtime_error("planes: " + name + ".bin holds " + std::to_string(static_cast<size_t>(file.tellg())) +
                               " bytes, its manifest line asks for " + std::to_string(want));
    file.seekg(0);
    p.bytes.resize(want);
    file.read(p.bytes.data(), static_cast<std::streamsize>(want));
    if (!file) throw std::runtime_error("planes: short read of " + name + ".bin");
    out[name] = std::move(p);
  }
  return out;
}

// `<dir>/<name>.bin` and one more line of `<dir>/<manifest>`
inline void write(const std::string& dir, const std::string& manifest, const std::string& name, const std::string& type,
                  const std::vector<int64_t>& dims, const void* data) {
  size_t bytes = width(type);
  for (int64_t d : dims) bytes *= static_cast<size_t>(d);
  std::ofstream file(dir + "/" + name + ".bin", std::ios::binary | std::ios::trunc);
  file.write(static_cast<const char*>(data), static_cast<std::streamsize>(bytes));
  file.close();
  if (!file) throw std::runtime_error("planes: cannot write " + name + ".bin");
  std::ofstream list(dir + "/" + manifest, std::ios::app);
  list << name << ' ' << type;
  for (int64_t d : dims) list << ' ' << d;
  list << '\n';
  list.close();
  if (!list) throw std::runtime_error("planes: cannot write " + manifest);
}

}  // namespace planes
