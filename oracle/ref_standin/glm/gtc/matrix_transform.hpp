// Stand-in for <glm/gtc/matrix_transform.hpp> — see glm/glm.hpp beside it.  Only rotate().
#pragma once
#include "../glm.hpp"

namespace glm {

// GLM: rotate(m, angle, v) builds the axis-angle rotation R from c = cos(angle), s = sin(angle),
// a = normalize(v) and t = (1 - c) a, with R[i][i] = c + t[i] a[i] and the off-diagonal terms
// t[i] a[j] +/- s a[k]; the result's first three columns are m0 R[i][0] + m1 R[i][1] + m2 R[i][2]
// (added left to right) and its fourth column is m3.
inline mat4 rotate(const mat4 &m, float angle, const vec3 &v) {
    const float c = std::cos(angle), s = std::sin(angle);
    const vec3 a = normalize(v);
    const vec3 t = (1.0f - c) * a;
    const float r00 = c + t.x * a.x, r01 = t.x * a.y + s * a.z, r02 = t.x * a.z - s * a.y;
    const float r10 = t.y * a.x - s * a.z, r11 = c + t.y * a.y, r12 = t.y * a.z + s * a.x;
    const float r20 = t.z * a.x + s * a.y, r21 = t.z * a.y - s * a.x, r22 = c + t.z * a.z;
    mat4 out;
    out[0] = m[0] * r00 + m[1] * r01 + m[2] * r02;
    out[1] = m[0] * r10 + m[1] * r11 + m[2] * r12;
    out[2] = m[0] * r20 + m[1] * r21 + m[2] * r22;
    out[3] = m[3];
    return out;
}

}  // namespace glm
