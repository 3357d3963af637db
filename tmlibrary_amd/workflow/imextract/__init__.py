"""imextract step: the planes of every site into channel image files."""
