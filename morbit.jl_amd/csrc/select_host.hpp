// What the host-only headers of the batched selection calls share: the defect a validation returns by value and
// the byte arena of a call.  No include of the project: the stand-alone checks under tools/ use it.
#pragma once
#include <cstddef>
#include <string>
#include <utility>

namespace mrbf {

struct Defect {
    int code = 0;  // 0, or -(1-based index of the invalid argument)
    std::string msg;
    explicit operator bool() const { return code != 0; }
};

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// pieces one behind the other, each rounded up to 256 bytes; the layout sets the marks of the two contiguous ranges that travel
struct ByteArena {
    size_t total = 0;
    size_t up_at = 0, up_end = 0, back_at = 0, back_end = 0;  // the packed upload, the read-back
    size_t take(size_t bytes) { return std::exchange(total, total + up256(bytes)); }
    size_t upload_bytes() const { return up_end - up_at; }
    size_t back_bytes() const { return back_end - back_at; }
};

}  // namespace mrbf
