// Stand-in for <assimp/Importer.hpp> (see ../README.md): ReadFile parses nothing, it hands back the
// scene the driver registered with standin_set_next_scene().
#pragma once
#include "scene.h"
namespace Assimp {
inline const aiScene *&standin_next_scene() {
    static const aiScene *scene = nullptr;
    return scene;
}
inline void standin_set_next_scene(const aiScene *scene) { standin_next_scene() = scene; }
class Importer {
   public:
    const aiScene *ReadFile(const char *, unsigned int) { return standin_next_scene(); }
    const char *GetErrorString() const { return "no scene registered with the stand-in importer"; }
};
}  // namespace Assimp
