// Stand-in for <assimp/postprocess.h> (see ../README.md): the flag names MeshEngine::load ors together.
// The stand-in importer ignores them; the values are distinct bits and carry no other meaning.
#pragma once
enum aiPostProcessSteps {
    aiProcess_Triangulate = 0x1,
    aiProcess_PreTransformVertices = 0x2,
    aiProcess_FlipUVs = 0x4,
    aiProcess_GenSmoothNormals = 0x8
};
