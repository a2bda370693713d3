// Stand-in for <glm/glm.hpp>, written for this project: just the float vector and matrix types and
// functions that the reference's translation units use, so that `make -C oracle ref` can compile those
// units unmodified (oracle/Makefile).  GLM itself is an empty submodule of the reference.
//
// Unlike tests/stubs/glm (types only, never linked) this header DEFINES ARITHMETIC.  Every operation
// rounds once and follows the reading tabulated in DESIGN_HISTORY.md §2: the generic (non-SIMD) code path
// of GLM's 0.9.9 series, as GLM's manual and public sources describe it.  These formulas therefore stay
// "stand-in readings": a build against this header pins the reference's own control flow, operand order,
// comparisons and constants, not GLM's last bits.
#pragma once
#include <cmath>
#include <cstddef>

namespace glm {

struct vec3;
struct vec4;

// Default construction gives zeros: GLM <= 0.9.8, or 0.9.9 with GLM_FORCE_CTOR_INIT (the
// kUvOfMeshesWithoutUvs reading; 0.9.9's plain default leaves the members indeterminate).
struct vec2 {
    float x, y;
    vec2() : x(0), y(0) {}
    template <typename A, typename B>
    vec2(A a, B b) : x(static_cast<float>(a)), y(static_cast<float>(b)) {}
    vec2(const vec3 &v);  // GLM: vec<2>(vec<3> const&) keeps x, y (implicit unless GLM_FORCE_EXPLICIT_CTOR)
};

struct vec3 {
    float x, y, z;
    vec3() : x(0), y(0), z(0) {}
    explicit vec3(float s) : x(s), y(s), z(s) {}
    template <typename A, typename B, typename C>
    vec3(A a, B b, C c) : x(static_cast<float>(a)), y(static_cast<float>(b)), z(static_cast<float>(c)) {}
    vec3(const vec4 &v);  // GLM: vec<3>(vec<4> const&) keeps x, y, z
    float &operator[](std::size_t i) { return i == 0 ? x : (i == 1 ? y : z); }
    const float &operator[](std::size_t i) const { return i == 0 ? x : (i == 1 ? y : z); }
};

struct vec4 {
    float x, y, z, w;
    vec4() : x(0), y(0), z(0), w(0) {}
    explicit vec4(float s) : x(s), y(s), z(s), w(s) {}  // GLM: a scalar fills every component
    template <typename A, typename B, typename C, typename D>
    vec4(A a, B b, C c, D d)
        : x(static_cast<float>(a)), y(static_cast<float>(b)), z(static_cast<float>(c)), w(static_cast<float>(d)) {}
    template <typename D>
    vec4(const vec3 &v, D d) : x(v.x), y(v.y), z(v.z), w(static_cast<float>(d)) {}
    float &operator[](std::size_t i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
    const float &operator[](std::size_t i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
    vec4 &operator+=(const vec4 &b) { x += b.x, y += b.y, z += b.z, w += b.w; return *this; }
    vec4 &operator*=(const vec4 &b) { x *= b.x, y *= b.y, z *= b.z, w *= b.w; return *this; }
};
typedef vec4 highp_vec4;

inline vec2::vec2(const vec3 &v) : x(v.x), y(v.y) {}
inline vec3::vec3(const vec4 &v) : x(v.x), y(v.y), z(v.z) {}

// GLM's operators are component-wise; a scalar operand is applied to each component as written
// (v / s divides each component, it does not multiply by a reciprocal).
inline vec2 operator+(const vec2 &a, const vec2 &b) { return vec2(a.x + b.x, a.y + b.y); }
inline vec2 operator*(const vec2 &a, float s) { return vec2(a.x * s, a.y * s); }

inline vec3 operator+(const vec3 &a, const vec3 &b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3 &a, const vec3 &b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3 &a, const vec3 &b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator/(const vec3 &a, const vec3 &b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline vec3 operator*(const vec3 &a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator*(float s, const vec3 &a) { return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator/(const vec3 &a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3 operator-(const vec3 &a) { return vec3(-a.x, -a.y, -a.z); }

inline vec4 operator+(const vec4 &a, const vec4 &b) { return vec4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
inline vec4 operator-(const vec4 &a, const vec4 &b) { return vec4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
inline vec4 operator*(const vec4 &a, const vec4 &b) { return vec4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
inline vec4 operator/(const vec4 &a, const vec4 &b) { return vec4(a.x / b.x, a.y / b.y, a.z / b.z, a.w / b.w); }
inline vec4 operator*(const vec4 &a, float s) { return vec4(a.x * s, a.y * s, a.z * s, a.w * s); }
inline vec4 operator/(const vec4 &a, float s) { return vec4(a.x / s, a.y / s, a.z / s, a.w / s); }

// GLM: dot(a, b) of vec3 forms the component-wise product, then adds x + y + z left to right.
inline float dot(const vec3 &a, const vec3 &b) {
    vec3 t = a * b;
    return t.x + t.y + t.z;
}
// GLM: cross(a, b) = (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y).
inline vec3 cross(const vec3 &a, const vec3 &b) {
    return vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
// GLM: length(v) = sqrt(dot(v, v)).
inline float length(const vec3 &v) { return std::sqrt(dot(v, v)); }
// GLM: normalize(v) = v * inversesqrt(dot(v, v)), and inversesqrt(x) = 1 / sqrt(x).
inline vec3 normalize(const vec3 &v) { return v * (1.0f / std::sqrt(dot(v, v))); }
// GLM: min(a, b) = (b < a) ? b : a and max(a, b) = (a < b) ? b : a, per component.
inline vec3 min(const vec3 &a, const vec3 &b) {
    return vec3((b.x < a.x) ? b.x : a.x, (b.y < a.y) ? b.y : a.y, (b.z < a.z) ? b.z : a.z);
}
inline vec3 max(const vec3 &a, const vec3 &b) {
    return vec3((a.x < b.x) ? b.x : a.x, (a.y < b.y) ? b.y : a.y, (a.z < b.z) ? b.z : a.z);
}

// Column-major 4x4; mat4(s) puts s on the diagonal.
struct mat4 {
    vec4 c[4];
    mat4() {}
    explicit mat4(float s) {
        c[0] = vec4(s, 0, 0, 0), c[1] = vec4(0, s, 0, 0), c[2] = vec4(0, 0, s, 0), c[3] = vec4(0, 0, 0, s);
    }
    vec4 &operator[](std::size_t i) { return c[i]; }
    const vec4 &operator[](std::size_t i) const { return c[i]; }
};
// GLM: mat4 * vec4 pairs the columns: (m0 v.x + m1 v.y) + (m2 v.z + m3 v.w).
inline vec4 operator*(const mat4 &m, const vec4 &v) {
    return (m[0] * v.x + m[1] * v.y) + (m[2] * v.z + m[3] * v.w);
}

}  // namespace glm
