// Stand-in for <assimp/scene.h>, written for this project (see ../README.md): data carriers only.
// The structs hold what the driver (oracle/ref_driver.cpp) assembles from plain arrays; member names
// are those of Assimp's public API that the reference reads.  No importer, no post-processing.
#pragma once
#ifndef VMX_REF_NO_GLOBAL_FLOAT_MATH
// Assimp's headers bring <math.h> in, which makes <cmath>'s float overloads visible in the global namespace:
// the default reading of the reference's unqualified cos / sin / floor / round on float arguments
// (DESIGN_HISTORY.md §2).  Built with VMX_REF_NO_GLOBAL_FLOAT_MATH those calls name C's double functions.
#include <math.h>
#endif

struct aiVector3D {
    float x, y, z;
};
struct aiFace {
    unsigned int mNumIndices;
    unsigned int *mIndices;
};
struct aiMesh {
    unsigned int mNumVertices = 0, mNumFaces = 0;
    aiVector3D *mVertices = nullptr;
    aiVector3D *mNormals = nullptr;
    aiVector3D *mTextureCoords[8] = {};
    aiFace *mFaces = nullptr;
    unsigned int mMaterialIndex = 0;
    bool HasTextureCoords(unsigned int index) const { return index < 8 && mTextureCoords[index] != nullptr && mNumVertices > 0; }
};
struct aiMaterial {};
struct aiTexture {};
struct aiLight {};
struct aiCamera {};
struct aiAnimation {};
struct aiScene {
    unsigned int mNumMeshes = 0, mNumMaterials = 0, mNumAnimations = 0, mNumTextures = 0, mNumLights = 0, mNumCameras = 0;
    aiMesh **mMeshes = nullptr;
    aiMaterial **mMaterials = nullptr;
    aiAnimation **mAnimations = nullptr;
    aiTexture **mTextures = nullptr;
    aiLight **mLights = nullptr;
    aiCamera **mCameras = nullptr;
    bool HasMeshes() const { return mMeshes != nullptr && mNumMeshes > 0; }
    bool HasAnimations() const { return mAnimations != nullptr && mNumAnimations > 0; }
};
