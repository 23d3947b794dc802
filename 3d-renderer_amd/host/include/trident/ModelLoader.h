// ModelLoader.h — geometry ingestion without Assimp.
//
// The reference imports models with Assimp 5.3.1 (Trident/src/Loader/ModelLoader.cpp:331, flags
// :26-37) and textures with stb_image (TextureLoader.cpp:290-304). Neither library is vendored in the
// reference snapshot, so this restates the parts of their behaviour that reach the renderer:
//   - ModelData / MeshInstance with the reference's field names (ModelLoader.h:21-40);
//   - Wavefront OBJ + MTL and glTF 2.0 (.gltf with external or data-URI buffers, .glb);
//   - aiProcess_Triangulate (polygon fans), aiProcess_JoinIdenticalVertices (exact attribute match),
//     aiProcess_GenSmoothNormals (normalised face normals summed per position when the file has none),
//     aiProcess_CalcTangentSpace (per-triangle UV tangents summed per vertex; the shaders never read
//     them, Default.frag:126-130), missing vertex colours = white (ModelLoader.cpp:436-443);
//   - material mapping: base colour (glTF baseColorFactor, MTL Kd + d), metallic / roughness (glTF
//     factors, MTL Pm / Pr; defaults 1 / 1 as ModelLoader.cpp:375-378), base-colour texture path;
//   - glTF node hierarchy baked into MeshInstance matrices (ModelLoader.cpp:505-540);
//   - glTF skins and animations -> ModelData::m_Skeleton / m_AnimationClips and the vertices' bone influences, by the
//     reference loader's rules (ModelLoader.cpp:87-183, :263-302, :545-628) applied to glTF's own structures:
//       bones: the first skin's joints in order, then the unseen joints of further skins, then animated nodes that
//         are no joint (identity inverse bind); m_SourceName = the node's name ("Node<i>" without one), m_Name =
//         trimmed with a leading "mixamorig:" removed; m_LocalBindTransform = the node's local matrix;
//         m_InverseBindMatrix from the first skin that lists the joint (identity without an accessor);
//       hierarchy: the parent is the nearest ancestor node that is a bone (transforms of nodes in between are
//         dropped, as in the reference); the root is the first parentless bone, bone 0 when there is none;
//       influences: JOINTS_0 (u8 / u16) / WEIGHTS_0 (float, or u8 / u16 taken as normalised) through the skin of
//         the node that instantiates the mesh, assigned as AssignBoneWeight does (free slot, else replace the
//         smallest when larger) and normalised as NormaliseBoneWeights does; a joint index beyond the skin refuses
//         the file;
//       clips: one per animation ("Clip<i>" without a name), key times in seconds, duration = the largest input
//         time, m_TicksPerSecond = 1000; one TransformChannel per target node with its T / R / S keys (a path the
//         node's channel already has keys for starts another channel for that node); LINEAR and STEP keys as they
//         are, CUBICSPLINE keys by their value element, all played linearly (one log line per file that loses
//         information this way); morph-target "weights" channels are skipped; an output accessor whose count
//         disagrees with its input refuses the file.
//     OBJ carries neither.
// Not restated: aiProcess_ImproveCacheLocality / OptimizeMeshes (they only reorder triangles or merge
// meshes; the rendered image differs at most at exact depth ties).
// Images: PNG (ImageDecoder.h: stb_image's PNG semantics on zlib) and binary PPM (P6) / PAM (P7, RGB /
// RGBA) decode to forced RGBA8 with stb's vertical flip for 2D textures (stbi_set_flip_vertically_on_load,
// TextureLoader.cpp:290-304) and without it for cube faces (:773); JPEG / TGA / BMP / HDR need stb and
// fail to load (the renderer then uses the default slot, as the reference does after a failed load).
#pragma once

#include <array>
#include <limits>
#include <string>
#include <vector>

#include "Animation.h"
#include "Scene.h"

namespace Trident {
namespace Loader {

struct MeshInstance {
    size_t m_MeshIndex = std::numeric_limits<size_t>::max();
    glm::mat4 m_ModelMatrix{1.0f};
    std::string m_NodeName;
};

struct ModelData {
    std::vector<Geometry::Mesh> m_Meshes;
    std::vector<Geometry::Material> m_Materials;
    std::vector<std::string> m_Textures;  // normalised paths referenced by materials
    std::vector<MeshInstance> m_MeshInstances;
    Animation::Skeleton m_Skeleton;
    std::vector<Animation::AnimationClip> m_AnimationClips;
};

class ModelLoader {
public:
    // Empty ModelData (and a logged error) when the file is missing, unsupported or malformed.
    static ModelData Load(const std::string& filePath);
};

class TextureLoader {
public:
    // RGBA8, rows flipped bottom-up like stb with flip-on-load; Width = 0 on failure.
    static TextureData Load(const std::string& filePath);
};

// SkyboxTextureLoader (TextureLoader.h / TextureLoader.cpp:334-830). An invalid (empty) result and a logged error when
// a file is missing, fails to decode, is truncated or differs in size from the other faces.
//   LDR faces: every face decoded to RGBA8 sRGB without the vertical flip, stored +X,-X,+Y,-Y,+Z,-Z.
//   EXR faces (all six paths end in .exr, LoadFromFileList :738-767): R16G16B16A16_SFLOAT, every channel through
//     FloatToHalf; single-part scanline files with HALF or FLOAT channels at sampling 1, compression NONE, RLE, ZIPS or
//     ZIP, either line order, rows top to bottom. Tiled, multi-part and deep files, UINT channels, PIZ and the later
//     codecs are refused by name (PIZ is a deviation from tinyexr: DESIGN.md §5l). A mix of .exr and other faces takes
//     the LDR loader, where the .exr face fails to decode, as in the reference.
//   KTX 1 (LoadFromKtx :417-563): little-endian, 6 faces; UNSIGNED_BYTE + SRGB8_ALPHA8 -> sRGB, UNSIGNED_BYTE + RGBA ->
//     UNORM, HALF_FLOAT or FLOAT + RGBA16F -> 8 bytes per texel (the FLOAT case is the reference's quirk, kept); the
//     key/value data is skipped; per level a size word (0 refused, otherwise ignored), six faces each padded to 4
//     bytes, the level padded to 4 bytes; dimensions halve with a floor of 1. Deviation: faces that are not square or
//     are wider than 16384 are refused (Vulkan would reject them; the reference never checks).
class SkyboxTextureLoader {
public:
    static CubemapTextureData LoadFromFaces(const std::array<std::string, 6>& facePaths);
    // TryMatchFaceIndex (:140-160) per file of the directory (sorted order): the first face whose
    // token (posx/px, negx/nx, ...) the lower-case stem contains; per face the first .exr candidate,
    // otherwise the first candidate (:384-411).
    static CubemapTextureData LoadFromDirectory(const std::string& directoryPath);
    static CubemapTextureData LoadFromKtx(const std::string& filePath);
    static CubemapTextureData LoadFromExrFaces(const std::array<std::string, 6>& facePaths);
    // The parsers over bytes in memory (`name` only labels the log): what the files' loaders call, and what
    // `make sky-check` runs over damaged files.
    static CubemapTextureData LoadKtxFromMemory(const uint8_t* data, size_t size, const std::string& name);
    static bool DecodeExrFaceFromMemory(const uint8_t* data, size_t size, const std::string& name, uint32_t& width,
                                        uint32_t& height, std::vector<uint16_t>& rgbaHalf);
};
// FloatToHalf (TextureLoader.cpp:162-204): drops 13 mantissa bits and adds one when the highest dropped bit is set (a
// tie rounds away from zero, not to even); a rebiased exponent below -10 gives a signed zero, subnormals come from the
// same shift-and-add, 31 or more gives infinity and a NaN keeps one mantissa bit.
uint16_t FloatToHalf(float value);

// Renderer::CreateSkyboxCubemap's discovery (Renderer.cpp:3830-3927) under `assetsDir` (the reference
// uses "Assets", relative to the working directory): Skyboxes/DefaultSkybox.ktx (when the file exists the search
// ends there, valid or not, like the reference's if / else at :3833-3921), else the
// Skyboxes/Default directory, else loose PNG faces in Skyboxes/ matched by the px/nx/... tokens (a
// file may fill every still-missing face whose token its stem contains), else invalid. `source`
// names what was used ("DefaultSkybox.ktx", "Default directory", "PNG fallback" or "").
CubemapTextureData DiscoverDefaultSkybox(const std::string& assetsDir, std::string& source);

// ApplicationLayer's DecomposeMatrixToTransform (ApplicationLayer.cpp:838-861): glm::decompose, then
// degrees(eulerAngles(normalize(q))). Returns false (and the default transform) when it fails.
bool DecomposeMatrixToTransform(const glm::mat4& modelMatrix, Transform& out);

}  // namespace Loader
}  // namespace Trident
