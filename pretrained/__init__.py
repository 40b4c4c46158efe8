"""Import-path shim for the reference's ``pretrained`` tree: the face parser of pretrained/face_parsing/ on the HIP engine."""
