// Stand-in for <assimp/cimport.h> (see ../README.md): the reference includes it and uses nothing of it.
#pragma once
